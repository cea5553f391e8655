"""Stand-alone timing of the fused forward.  Default: the fused HIP forward against the graph-replayed torch form.
--weights fp8: the fp8-weight form against the two fp16 forms (4-wave: HM_NET_WAVES=4, 8-wave default) in one process, the forms
alternated round by round, device events over >= 20 launches each; writes ms per launch, TFLOP/s and the weight bytes a position
streams (computed from the packed buffers' shapes) to --out.
--acts fp8: the same alternation for the form on native FP8 MFMA (e4m3 activations and weights, 8 waves; scales calibrated on random
planes) against the fp8-weight form (4 waves) and the fp16 8-wave default.
--pair: the same alternation for the pair form (two positions per workgroup) of RISEv3-small against the two fp16 forms; the
384-channel network, which has no pair form, is left out.
--split T: the same alternation for the team form (T = 2 or 3 workgroups per position) of the deployed 384-channel network against
the two fp16 forms, at the row counts of one game's search (8, 16, 64, 128 by default); RISEv3-small has no team form.
--xboard: cross_board_rise_v33() (trunk in features form + attention tail, two launches) against rise_v33() (8-wave form), alternated
in the same way at 8, 64 and 512 rows by default; the tail's own time is reported by difference of the two."""
import argparse, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, hivemind_amd as hm
from hivemind_amd import net as N

ap = argparse.ArgumentParser()
ap.add_argument("--weights", choices=("fp16", "fp8"), default="fp16")
ap.add_argument("--acts", choices=("fp16", "fp8"), default="fp16")
ap.add_argument("--pair", action="store_true")
ap.add_argument("--split", type=int, default=0, choices=(0, 2, 3))
ap.add_argument("--xboard", action="store_true")
ap.add_argument("--rows", type=int, nargs="+", default=None)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
alternate = args.pair or args.split or args.weights == "fp8" or args.acts == "fp8"
if args.out is None: args.out = "net_xboard.json" if args.xboard else "net_pair.json" if args.pair else "net_split.json" if args.split else "net_a8.json" if args.acts == "fp8" else "net_fp8.json"
hm.init(0)
torch.manual_seed(0)
out = {}


def timed(f, x, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): f(x)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


if args.xboard:
    forms = {"xboard": N.FusedNet(N.cross_board_rise_v33()), "rise_v33": N.FusedNet(N.rise_v33())}
    for n in args.rows or (8, 64, 512):
        x = torch.rand((n, 74, 8, 8), device="cuda").half()
        for f in forms.values():
            for _ in range(3): f(x)
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items(): ms[k].append(timed(f, x, args.iters))
        res = {k: dict(ms=sum(v) / len(v), ms_min=min(v), ms_max=max(v), launches=len(v) * args.iters) for k, v in ms.items()}
        res["tail_ms_by_difference"] = res["xboard"]["ms"] - res["rise_v33"]["ms"]
        out[f"rows_{n}"] = res
        print(n, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    sys.exit(0)

for name, mk in (("small", N.rise_v3_small), ("full", N.rise_v33))[1 if args.split else 0:1 if args.pair else 2]:
    model = mk()
    fl = N.flops_per_position(model)
    if alternate:
        forms = {}
        first = ("pair", None, "fp16") if args.pair else (f"split{args.split}", None, "fp16") if args.split else ("fp8_w4", None, "fp8")
        others = (("fp8_w4", None, "fp8"), ("fp16_w8", "8", "fp16")) if args.acts == "fp8" else (("fp16_w4", "4", "fp16"), ("fp16_w8", "8", "fp16"))
        if args.acts == "fp8":
            first = ("a8_w8", None, "fp8")
            calib = dict(acts="fp8", calibration=torch.rand((64, 74, 8, 8), device="cuda"))
        for label, waves, w in (first, *others):
            if waves: os.environ["HM_NET_WAVES"] = waves              # read once, by hm_net_create
            forms[label] = N.FusedNet(model, weights=w, pair=label == "pair", split=args.split if label.startswith("split") else 0, **(calib if label == "a8_w8" else {}))
        os.environ.pop("HM_NET_WAVES", None)
        wbytes = {k: int(f.wh.numel() * 2 + (f.w8.numel() if f.weights == "fp8" else 0)) for k, f in forms.items()}
        for n in args.rows or ((8, 16, 64, 128) if args.split else (64, 512, 2048)):
            x = torch.rand((n, 74, 8, 8), device="cuda").half()
            for f in forms.values():
                for _ in range(3): f(x)
            torch.cuda.synchronize()
            ms = {k: [] for k in forms}
            for _ in range(args.rounds):                              # alternate the forms: drift hits all of them alike
                for k, f in forms.items(): ms[k].append(timed(f, x, args.iters))
            res = {k: dict(ms=sum(v) / len(v), ms_min=min(v), ms_max=max(v), launches=len(v) * args.iters,
                           tflops=n * fl / (sum(v) / len(v) * 1e-3) / 1e12, weight_bytes_per_position=wbytes[k]) for k, v in ms.items()}
            out[f"{name}_{n}"] = res
            print(name, n, json.dumps(res), flush=True)
        continue
    fused = N.FusedNet(model)
    for n in args.rows or (64, 512, 2048, 8192):
        x = torch.rand((n, 74, 8, 8), device="cuda").half()
        inf = N.InferenceNet(model).capture(n)
        res = {}
        for label, f in (("fused", fused), ("torch_graph", inf)):
            for _ in range(3): f(x)
            torch.cuda.synchronize()
            ms = timed(f, x, 20)
            res[label] = dict(ms=ms, tflops=n * fl / (ms * 1e-3) / 1e12)
        out[f"{name}_{n}"] = res
        print(name, n, json.dumps(res), flush=True)
if alternate:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
if args.split and forms[f"split{args.split}"].split_error():
    sys.exit("the team form gave up a launch")
