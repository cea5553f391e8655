"""The fused forward on native FP8 MFMA (FusedNet(weights="fp8", acts="fp8"), hm_net_create_a8) against a plain fp32 torch reference
that applies the kernel's numerics contract (hm_net_a8_device.hpp): weights snapped to the e4m3 grid, activations quantised with torch's
own float8_e4m3fn cast at exactly the kernel's points.

The bound is measured from the reference alone.  An fp16-rounded intermediate near an e4m3 rounding boundary flips a code, so the
reference is evaluated twice: (a) in plain fp32, (b) with every tensor the kernel keeps in fp16 rounded through fp16; per case and head
bound = max(1e-3 * max(1, |ref|max), 2 * |a - b|max) (the kernel's flips are a second draw of the process that separates a and b), and
the kernel must lie within it of (a).  The cost of quantisation against the unsnapped fp32 model is recorded, not asserted.

Case c384 sets the chunk of the expansion to 192 channels (HM_NET_COP_CHUNK), so that its cop = 320 runs as two chunks, the second one
(128) carried into the projection's accumulators; the kernel's own chunk there would be 320.  The deployed network ("full") chunks by
itself, with last chunks of 32 (mod 64) channels."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("value", "pi_a", "pi_b", "wdl", "moves_left")


def _model(case):
    from hivemind_amd import net as N
    from test_gpu_net import _randomise_bn
    torch.manual_seed(0)
    model = {"c128": lambda: N.RiseV3(128, 160, 32, [3], [True], 8, 256),
             "c384": lambda: N.RiseV3(384, 320, 0, [5, 3], [False, True], 16, 512),
             "small": N.rise_v3_small, "full": N.rise_v33}[case.split("-")[0]]()
    _randomise_bn(model, 1)
    return model.eval()


def _q(x, sa):                      # the quantisation step, dequantised
    return (x / sa).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * sa


@torch.no_grad()
def _reference(m, planes, sa, half):
    """The snapped model `m` in fp32 with the kernel's quantisation points; half: the kernel's fp16 tensors rounded through fp16."""
    r = (lambda t: t.half().float()) if half else (lambda t: t)
    n = planes.shape[0]
    x = m.body_spatial[0](planes)                                        # stem: codes and the fp16 master from the same fp32 value
    xq, x = _q(x, sa[0]), r(x)
    for i, blk in enumerate(list(m.body_spatial)[1:]):
        if blk.se_type:                                                  # the gate works on the master; its product is requantised
            x = blk.se(x)
            xq, x = _q(x, sa[2 * i]), r(x)
        y1 = r(blk.body[:3](xq))                                         # expand -> Y1, fp16
        y2 = _q(blk.body[3:6](y1), sa[2 * i + 1])                        # depthwise: codes from the fp32 sum
        x = x + blk.body[6:](y2)                                         # residual on the master, codes from the fp32 sum
        xq, x = _q(x, sa[2 * i + 2]), r(x)
    vh, ph = m.value_head, m.policy_heads
    v = r(vh.body(xq)).reshape(n, -1)                                    # value conv output, fp16
    wdl, plys = vh.body_wdl(v), vh.body_plys(v)
    sm = torch.softmax(wdl, dim=1)
    s = _q(ph.shared_body(xq), sa[-1])
    pa, pb = (p(s).reshape(n, -1) for p in ph.board_projections)
    return tuple(r(t) for t in (sm[:, 2] - sm[:, 0], pa, pb, wdl, plys.reshape(n)))


def _planes(hm, seed):
    import oracle_py as O
    return hm.board_to_planes(hm.to_device(O.random_positions(seed, 64, 100)), "f16")


@pytest.mark.parametrize("case", ["c128", "c384", "c384-clamped", "small", "full"])
def test_a8_forward_matches_fake_quantised_reference(hm, case, monkeypatch):
    from hivemind_amd import net as N
    from test_gpu_net_fp8 import _snap
    if case.startswith("c384"):
        monkeypatch.setenv("HM_NET_COP_CHUNK", "192")
    planes = _planes(hm, 3)
    model = _model(case)
    sa = N.calibrate_act_scales(model, planes)
    if case.endswith("clamped"):                                         # every scale / 8: the clamp works in the kernel and the reference alike
        sa = [s / 8 for s in sa]
    # recorded, not asserted: what e4m3 weights and activations cost on the unsnapped model
    with torch.no_grad():
        ref = model.cuda().float()(planes.float())
    got = N.FusedNet(model, weights="fp8", acts="fp8", act_scales=sa)(planes)
    torch.cuda.synchronize()
    report = {}
    for nme, r, g in zip(NAMES, ref, got):
        r = r.float().reshape(g.shape)
        report[nme] = dict(quant_max_abs_err=float((g.float() - r).abs().max()), logit_scale=float(r.abs().max()))
        if nme.startswith("pi_"):
            report[nme]["quant_argmax_agreement"] = float((g.float().argmax(1) == r.argmax(1)).float().mean())
    # asserted: the kernel on grid weights against the fake-quantised reference
    snapped = _snap(_model(case)).cuda().float()
    ref_a, ref_b = _reference(snapped, planes.float(), sa, False), _reference(snapped, planes.float(), sa, True)
    got = N.FusedNet(snapped, weights="fp8", acts="fp8", act_scales=sa)(planes)
    torch.cuda.synchronize()
    failed = []
    for nme, a, b, g in zip(NAMES, ref_a, ref_b, got):
        a, b, g = a.reshape(g.shape), b.reshape(g.shape), g.float()
        bound = max(1e-3 * max(1.0, float(a.abs().max())), 2 * float((a - b).abs().max()))
        err_a, err_b = float((g - a).abs().max()), float((g - b).abs().max())
        report[nme].update(err_a=err_a, err_b=err_b, bound=bound)
        print(case, nme, "|kernel-a|", err_a, "|kernel-b|", err_b, "bound", bound)
        assert bool(torch.isfinite(g).all()), (case, nme)
        if not err_a <= bound:
            failed.append((nme, err_a, bound))
    print("numerics[%s] fp8-activation forward: %s" % (case, json.dumps(report)))
    out_dir = os.environ.get("HM_NUMERICS_DIR", "numerics_out")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(report, open(os.path.join(out_dir, f"net_numerics_a8_{case}.json"), "w"), indent=1)
    assert not failed, (case, failed)


def test_a8_rows_do_not_depend_on_the_batch(hm):
    from hivemind_amd import net as N
    planes = _planes(hm, 4)
    fused = N.FusedNet(_model("c128"), weights="fp8", acts="fp8", calibration=planes)
    got = [t.clone() for t in fused(planes)]
    for n in (1, 7):
        for a, b in zip(fused(planes[:n].contiguous()), got):
            assert torch.equal(a, b[:n])


def test_a8_ragged_groups(hm):
    from hivemind_amd import net as N
    planes = _planes(hm, 5)
    fused = N.FusedNet(_model("c128"), weights="fp8", acts="fp8", calibration=planes)
    dense = [t.clone() for t in fused(planes)]
    counts = torch.tensor([8, 0, 3, 1, 7, 8, 0, 5], dtype=torch.int32, device="cuda")
    out = tuple(torch.full_like(t, 7.0) for t in dense)
    fused(planes, out=out, group_rows=counts, group=8)
    torch.cuda.synchronize()
    live = torch.tensor([r % 8 < counts[r // 8].item() for r in range(64)]).cuda()
    for d, o in zip(dense, out):
        assert torch.equal(o[live], d[live])
        assert bool((o[~live] == 7.0).all())


def test_a8_network_refusals(hm):
    import oracle_py as O
    from hivemind_amd import net as N
    fused = N.FusedNet(_model("c128"), weights="fp8", acts="fp8", calibration=_planes(hm, 1))
    eng = hm.SearchEngine(4, 200)
    eng.set_games(O.random_positions(1, 4, 60))
    eng.begin_search(16)
    with pytest.raises(hm.HivemindError, match="cannot be the evaluator"):
        eng.search_persistent(fused)
    with pytest.raises(NotImplementedError):
        fused.save("unused.hmnet")
