"""Host side of FusedNet(weights="fp8", acts="fp8"): the K = 64 operand packing, the calibrated power-of-two activation scales, the
quantisation step and the combinations the constructor refuses (all before any device work)."""
import math

import pytest
import torch


def test_pack_frag8x64_layout():
    """[K/64][tile][lane][32]: lane l holds W[kstep*64 + 32*(l>>5) + j][tile*32 + (l&31)]."""
    from hivemind_amd.net import _pack_frag8x64
    w = (torch.arange(128 * 64) % 251).to(torch.uint8).reshape(128, 64)
    p = _pack_frag8x64(w).reshape(2, 2, 64, 32)                          # kstep, tile, lane, j
    lane = torch.arange(64)
    for ks in range(2):
        for tile in range(2):
            for j in (0, 1, 15, 16, 31):
                assert torch.equal(p[ks, tile, :, j], w[ks * 64 + 32 * (lane >> 5) + j, tile * 32 + (lane & 31)])
    assert torch.equal(p.reshape(-1).sort().values, w.reshape(-1).sort().values)       # a permutation: the round trip loses nothing


def test_calibrated_scales_and_codes():
    from hivemind_amd import net as N
    torch.manual_seed(1)
    model = N.RiseV3(128, 160, 32, [3, 5], [True, False], 8, 256).eval()
    planes = torch.rand(4, 74, 8, 8)
    sa = N.calibrate_act_scales(model, planes)
    assert len(sa) == 2 * 2 + 2
    with torch.no_grad():
        x = model.body_spatial[0](planes)
        x = model.body_spatial[1].se(x)
    amax0 = float(x.abs().max())
    assert sa[0] >= 2 * amax0 / 448 and sa[0] < 4 * amax0 / 448
    for s in sa:
        assert s > 0 and math.frexp(s)[0] == 0.5                         # a power of two
    # the step never draws the NaN code, in range or far out of it
    v = torch.cat([x.flatten(), torch.tensor([1e30, -1e30, 448.0 * sa[0], 464.0 * sa[0], -500.0 * sa[0], 0.0])])
    codes = N.quantize_act_e4m3(v, sa[0])
    assert not bool(((codes & 0x7F) == 0x7F).any())
    assert int(codes[-3]) == 0x7E and int(codes[-2]) == 0xFE             # clamped to +-448


@pytest.mark.parametrize("kw", [
    dict(acts="fp8", calibration=True),                                  # without weights="fp8"
    dict(weights="fp8", acts="fp8"),                                     # without calibration or scales
    dict(weights="fp8", acts="fp8", calibration=True, pair=True),
    dict(weights="fp8", acts="fp8", calibration=True, split=2),
    dict(weights="fp8", acts="fp8", calibration=True, xboard=True),
    dict(weights="fp8", acts="fp8", calibration=True, channels=64),
    dict(weights="fp8", acts="fp8", act_scales=[1.0, 0.5, 3.0, 1.0]),    # not a power of two
])
def test_refusals(kw):
    from hivemind_amd import net as N
    kw = dict(kw)
    ch = kw.pop("channels", 128)
    model = (N.CrossBoardRiseV3(128, 128, 32, [3], [False], 8, 256, attention_layers=1) if kw.pop("xboard", False)
             else N.RiseV3(ch, 128, 32, [3], [False], 8, 256))
    if kw.get("calibration"):
        kw["calibration"] = torch.rand(2, 74, 8, 8)
    with pytest.raises(ValueError):
        N.FusedNet(model, device="cpu", **kw)
