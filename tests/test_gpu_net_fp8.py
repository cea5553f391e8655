"""The fused forward with FP8 (e4m3) weights (FusedNet(weights="fp8"), hm_net_create_w8) against a plain fp32 PyTorch reference.
Quantisation is taken out of the comparison: the model is first snapped to the e4m3 grid with torch's own float8 cast, so the kernel
multiplies exactly the reference's weights and the project's bound (north_star: value / policy logits within 1e-3 of the logit scale,
as in test_gpu_net.py) applies unchanged.  The cost of quantising an unsnapped model is recorded, not asserted."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("value", "pi_a", "pi_b", "wdl", "moves_left")


def _model(name):
    from hivemind_amd import net as N
    from test_gpu_net import _randomise_bn
    torch.manual_seed(0)
    model = N.rise_v3_small() if name == "small" else N.rise_v33()
    _randomise_bn(model, 1)
    return model.eval()


def _grid(w):                      # per output channel: scale amax / 448, to e4m3 and back
    s = w.abs().flatten(1).amax(1).clamp_min(1e-30).view(-1, 1, 1, 1) / 448.0
    return (w / s).to(torch.float8_e4m3fn).float() * s


@torch.no_grad()
def _snap(model):
    """Every conv(+BN) FusedNet quantises: folded, snapped to the grid, written back with an identity BatchNorm."""
    vh, ph = model.value_head, model.policy_heads
    pairs = [(vh.body[0], vh.body[1]), (ph.shared_body[0], ph.shared_body[1])]
    for blk in list(model.body_spatial)[1:]:
        pairs += [(blk.body[0], blk.body[1]), (blk.body[6], blk.body[7])]
    for conv, bn in pairs:
        k = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        conv.weight.copy_(_grid(conv.weight * k.view(-1, 1, 1, 1)))
        bn.bias.copy_(bn.bias - bn.running_mean * k)
        bn.weight.fill_(1.0); bn.running_mean.zero_(); bn.running_var.fill_(1.0 - bn.eps)     # fold factor exactly 1.0
    for proj in ph.board_projections:
        proj.weight.copy_(_grid(proj.weight))
    return model


def _planes(hm, seed):
    import oracle_py as O
    return hm.board_to_planes(hm.to_device(O.random_positions(seed, 64, 100)), "f16")


@pytest.mark.parametrize("name", ["small", "full"])
def test_fp8_forward_matches_fp32_reference(hm, name):
    from hivemind_amd import net as N
    planes = _planes(hm, 3)
    # recorded, not asserted: what e4m3 weights cost on the unsnapped model
    model = _model(name)
    with torch.no_grad():
        ref = model.cuda().float()(planes.float())
    got = N.FusedNet(model, weights="fp8")(planes)
    torch.cuda.synchronize()
    report = {}
    for nme, r, g in zip(NAMES, ref, got):
        report[nme] = dict(max_abs_err=float((g.float() - r.float().reshape(g.shape)).abs().max()), logit_scale=float(r.abs().max()))
        if nme.startswith("pi_"):
            report[nme]["argmax_agreement"] = float((g.float().argmax(1) == r.reshape(g.shape).argmax(1)).float().mean())
    print("\nnumerics[%s] fp8-weight forward vs fp32 torch (unsnapped): %s" % (name, json.dumps(report)))
    out_dir = os.environ.get("HM_NUMERICS_DIR", "numerics_out")        # where the recorded figures go
    os.makedirs(out_dir, exist_ok=True)
    json.dump(report, open(os.path.join(out_dir, f"net_numerics_fp8_{name}.json"), "w"), indent=1)
    # asserted: the kernel on grid weights against the same weights in fp32
    snapped = _snap(_model(name))
    with torch.no_grad():
        ref = snapped.cuda().float()(planes.float())
    fused = N.FusedNet(snapped, weights="fp8")
    got = fused(planes)
    torch.cuda.synchronize()
    for nme, r, g in zip(NAMES, ref, got):
        r = r.float().reshape(g.shape)
        err, scale = float((g.float() - r).abs().max()), max(1.0, float(r.abs().max()))
        print(name, nme, "max_abs_err", err, "scale", scale)
        assert bool(torch.isfinite(g).all()), (name, nme)
        assert err / scale < 1e-3, (name, nme, err, scale)
    for n in (1, 7):                                                    # batch independence
        for a, b in zip(fused(planes[:n].contiguous()), got):
            assert torch.equal(a, b[:n])
    with pytest.raises(NotImplementedError):
        fused.save("unused.hmnet")


def test_fp8_ragged_groups(hm):
    from hivemind_amd import net as N
    planes = _planes(hm, 5)
    fused = N.FusedNet(_model("small"), weights="fp8")
    dense = [t.clone() for t in fused(planes)]
    counts = torch.tensor([8, 0, 3, 1, 7, 8, 0, 5], dtype=torch.int32, device="cuda")
    out = tuple(torch.full_like(t, 7.0) for t in dense)
    fused(planes, out=out, group_rows=counts, group=8)
    torch.cuda.synchronize()
    live = torch.tensor([r % 8 < counts[r // 8].item() for r in range(64)]).cuda()
    for d, o in zip(dense, out):
        assert torch.equal(o[live], d[live])
        assert bool((o[~live] == 7.0).all())


def test_fp8_network_is_refused_by_the_single_launch_search(hm):
    import oracle_py as O
    from hivemind_amd import net as N
    fused = N.FusedNet(_model("small"), weights="fp8")
    eng = hm.SearchEngine(4, 200)
    eng.set_games(O.random_positions(1, 4, 60))
    eng.begin_search(16)
    with pytest.raises(hm.HivemindError, match="cannot be the evaluator"):
        eng.search_persistent(fused)
    assert hm.lib.hm_last_error()
