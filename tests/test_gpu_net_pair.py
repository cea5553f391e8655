"""The pair form of the fused forward (FusedNet(pair=True): two positions per workgroup, M = 128 rows per weight fragment) against
the plain fp32 PyTorch model (the bound of test_gpu_net.py: max_abs_err / max(1, max|ref|) < 1e-3 per head) and, bit for bit,
against the one-position form: whatever row a position is paired with, and whether its partner is live or dead."""
import pytest
import torch

from test_gpu_net import _randomise_bn

pytestmark = pytest.mark.gpu


def _model(name):
    from hivemind_amd import net as N
    torch.manual_seed(0)
    # "c64k5": two channel tiles (waves 2 and 3 own none), a 5x5 depthwise, ECA; "small": C = 128, ECA, chunked blocks with a 32-channel tail
    model = N.rise_v3_small() if name == "small" else N.RiseV3(64, 64, 32, [3, 5, 3, 3], [False, True, False, True], 8, 256)
    _randomise_bn(model, 1)
    return model.eval()


def _planes(hm, seed, n):
    import oracle_py as O
    return hm.board_to_planes(hm.to_device(O.random_positions(seed, n, 120)), "f16")


@pytest.mark.parametrize("name", ["small", "c64k5"])
def test_pair_matches_reference_and_one_position_form(hm, name):
    from hivemind_amd import net as N
    model = _model(name)
    planes = _planes(hm, 3, 33)
    with torch.no_grad():
        ref = model.cuda().float()(planes.float())
    pair = N.FusedNet(model, pair=True)
    got = [t.clone() for t in pair(planes)]
    one = N.FusedNet(model)(planes)
    torch.cuda.synchronize()
    for nme, r, g, o in zip(("value", "pi_a", "pi_b", "wdl", "moves_left"), ref, got, one):
        r = r.float().reshape(g.shape)
        scale = max(1.0, float(r.abs().max()))
        err = float((g.float() - r).abs().max())
        print(name, nme, "max_abs_err", err, "scale", scale)
        assert err / scale < 1e-3, (name, nme, err, scale)
        assert torch.equal(g, o), (name, nme)
    for n in (1, 2, 7):
        for a, b in zip(pair(planes[:n].contiguous()), got):
            assert torch.equal(a, b[:n]), (name, n)
    for a, b in zip(pair(planes.flip(0).contiguous()), got):            # every row with another partner
        assert torch.equal(a, b.flip(0)), name


B_PATTERN = [1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0,
             0, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("group,counts", [(8, [8, 0, 3, 1, 7, 8, 0, 5]), (1, B_PATTERN)], ids=["groups_of_8", "single_rows"])
def test_pair_ragged_groups(hm, group, counts):
    from hivemind_amd import net as N
    if group == 1:
        kinds = [(counts[i], counts[i + 1]) for i in range(0, 64, 2)]
        assert kinds.count((1, 1)) >= 1 and kinds.count((0, 0)) >= 1 and kinds.count((1, 0)) >= 4 and kinds.count((0, 1)) >= 4
    planes = _planes(hm, 5, 64)
    pair = N.FusedNet(_model("small"), pair=True)
    dense = [t.clone() for t in pair(planes)]
    out = tuple(torch.full_like(t, 7.0) for t in dense)
    pair(planes, out=out, group_rows=torch.tensor(counts, dtype=torch.int32, device="cuda"), group=group)
    torch.cuda.synchronize()
    live = torch.tensor([r % group < counts[r // group] for r in range(64)]).cuda()
    for d, o in zip(dense, out):
        assert torch.equal(o[live], d[live])
        assert bool((o[~live] == 7.0).all())


def test_pair_refusals(hm):
    from hivemind_amd import net as N
    with pytest.raises(hm.HivemindError):
        N.FusedNet(N.rise_v33(), pair=True)
    with pytest.raises(ValueError):
        N.FusedNet(N.rise_v3_small(), weights="fp8", pair=True)
