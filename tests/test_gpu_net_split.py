"""The team form of the fused forward (FusedNet(split=T): T = 2 or 3 workgroups carry one position of the 384-channel trunk) against the
plain fp32 PyTorch model (the bound of test_gpu_net.py: max_abs_err / max(1, max|ref|) < 1e-3 per head; the same arithmetic measures
2e-4 there, and a CPU fp16 run of "c384" on random planes gave at most 2.0e-4) and, bit for bit, against the one-position form."""
import functools

import pytest
import torch

from test_gpu_net import _randomise_bn

pytestmark = pytest.mark.gpu
HEADS = ("value", "pi_a", "pi_b", "wdl", "moves_left")


@functools.lru_cache(maxsize=None)
def _model(name):
    from hivemind_amd import net as N
    torch.manual_seed(0)
    # "c384": 19 expanded tiles (3x3, no ECA: uneven shares 10/9 and 7/6/6), then 36 tiles (5x5, ECA: the widest block of the deployed
    # net; a member's slice of 576 / 384 channels exceeds one LDS chunk of 256); "v33": all 15 block widths, the odd 19 and 25 tiles among them
    model = N.rise_v33() if name == "v33" else N.RiseV3(384, 608, 544, [3, 5], [False, True], 16, 512)
    _randomise_bn(model, 1)
    return model.eval()


def _planes(hm, seed, n):
    import oracle_py as O
    return hm.board_to_planes(hm.to_device(O.random_positions(seed, n, 120)), "f16")


@functools.lru_cache(maxsize=None)
def _expected(hm, name, seed, n):
    """(planes, fp32 reference heads, heads of the default one-position form), computed once per network"""
    from hivemind_amd import net as N
    planes = _planes(hm, seed, n)
    with torch.no_grad():
        ref = [t.float() for t in _model(name).cuda().float()(planes.float())]
    one = [t.clone() for t in N.FusedNet(_model(name))(planes)]
    torch.cuda.synchronize()
    return planes, ref, one


@pytest.mark.parametrize("name,T", [("c384", 2), ("c384", 3), ("v33", 3)])
def test_split_matches_reference_and_one_position_form(hm, name, T):
    from hivemind_amd import net as N
    planes, ref, one = _expected(hm, name, 3, 33)
    net = N.FusedNet(_model(name), split=T)
    got = [t.clone() for t in net(planes)]
    torch.cuda.synchronize()
    for nme, r, g, o in zip(HEADS, ref, got, one):
        r = r.reshape(g.shape)
        scale = max(1.0, float(r.abs().max()))
        err = float((g.float() - r).abs().max())
        print(name, T, nme, "max_abs_err", err, "scale", scale)
        assert err / scale < 1e-3, (name, T, nme, err, scale)
        assert torch.equal(g, o), (name, T, nme)
    for n in (1, 2, 7):
        for a, b in zip(net(planes[:n].contiguous()), got):
            assert torch.equal(a, b[:n]), (name, T, n)
    assert net.split_error() == 0


def test_split_few_teams_ragged_groups_repeated_launches(hm, monkeypatch):
    from hivemind_amd import net as N
    monkeypatch.setenv("HM_NET_MAX_BLOCKS", "7")       # two teams of three (a capacity that is no multiple of T), 32 rows each
    net = N.FusedNet(_model("c384"), split=3)
    monkeypatch.delenv("HM_NET_MAX_BLOCKS")
    planes, _, one = _expected(hm, "c384", 5, 64)
    dense = [t.clone() for t in net(planes)]
    for h, d, o in zip(HEADS, dense, one):
        assert torch.equal(d, o), h
    counts = [8, 0, 3, 1, 7, 8, 0, 5]
    out = tuple(torch.full_like(t, 7.0) for t in dense)
    net(planes, out=out, group_rows=torch.tensor(counts, dtype=torch.int32, device="cuda"), group=8)
    live = torch.tensor([r % 8 < counts[r // 8] for r in range(64)]).cuda()
    for d, o in zip(dense, out):
        assert torch.equal(o[live], d[live])
        assert bool((o[~live] == 7.0).all())
    outs = [tuple(torch.zeros_like(t) for t in dense) for _ in range(3)]
    for o in outs:                                     # back to back, no host sync in between
        net(planes, out=o)
    for o in outs:
        for a, d in zip(o, dense):
            assert torch.equal(a, d)
    cap = tuple(torch.zeros_like(t) for t in dense)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net(planes, out=cap)
    for _ in range(2):
        graph.replay()
        for a, d in zip(cap, dense):
            assert torch.equal(a, d)
        for a in cap:
            a.zero_()
    assert net.split_error() == 0


def test_split_refusals(hm):
    from hivemind_amd import net as N
    with pytest.raises(hm.HivemindError):
        N.FusedNet(N.rise_v3_small(), split=3)
    with pytest.raises(hm.HivemindError):
        N.FusedNet(_model("c384"), split=4)
    with pytest.raises(ValueError):
        N.FusedNet(_model("c384"), weights="fp8", split=3)
    with pytest.raises(ValueError):
        N.FusedNet(_model("c384"), pair=True, split=3)
