"""The 4-wave stand-alone form of the fused forward (HM_NET_WAVES=4: narrow_position4, the evaluator body of the single-launch search)
against the default 8-wave form, bit for bit on all five heads: the header of narrow_position4 promises it, and the shared phases of
hm_net_phases.hpp (ECA gate, value tail) are where it is kept."""
import pytest
import torch

from test_gpu_net_pair import _model, _planes

pytestmark = pytest.mark.gpu
HEADS = ("value", "pi_a", "pi_b", "wdl", "moves_left")


@pytest.mark.parametrize("name", ["c64k5", "small"])
def test_four_wave_form_equals_eight_wave_form(hm, name, monkeypatch):
    from hivemind_amd import net as N
    model = _model(name)
    planes = _planes(hm, 3, 5)
    eight = N.FusedNet(model)
    monkeypatch.setenv("HM_NET_WAVES", "4")
    four = N.FusedNet(model)
    monkeypatch.delenv("HM_NET_WAVES")
    want = [t.clone() for t in eight(planes)]
    got = [t.clone() for t in four(planes)]
    torch.cuda.synchronize()
    for h, w, g in zip(HEADS, want, got):
        assert torch.equal(g, w), (name, h)
    for n in (1, 3):                                    # a row's heads do not depend on the batch it came in
        for net in (eight, four):
            for h, a, w in zip(HEADS, net(planes[:n].contiguous()), want):
                assert torch.equal(a, w[:n]), (name, h, n)
