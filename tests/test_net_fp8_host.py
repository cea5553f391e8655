"""Host side of the FP8 (e4m3) weight format of the fused forward: per-channel quantisation and the fragment-pair packing."""
import pytest
import torch


@pytest.mark.parametrize("k", [32, 1152])
def test_quantize_e4m3(k):
    from hivemind_amd.net import quantize_e4m3
    g = torch.Generator().manual_seed(7)
    w = torch.randn(k, 64, generator=g)
    w[:, 3] = 0.0                      # an all-zero column (the padded columns of the value conv / policy projection)
    w[k // 2, 5] = 1.0e4               # a single huge outlier
    codes, scale = quantize_e4m3(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (64,)
    assert not bool(((codes & 0x7F) == 0x7F).any())                     # never the e4m3 NaN pattern
    assert float(scale[3]) == 1.0 and not bool(codes[:, 3].any())
    deq = codes.view(torch.float8_e4m3fn).float() * scale
    amax = w.abs().amax(dim=0)
    # e4m3 spacing in the top binade is 32 codes-units: error <= 16 * scale = amax / 28, plus fp32 rounding
    assert bool(((w - deq).abs() <= amax / 27).all())


def test_pack_frag8_layout():
    """[kstep/2][tile][lane][2][8]: lane l holds W[ks*16 + 8*(l>>5) + j][tile*32 + (l&31)] for k-steps 2p and 2p + 1."""
    from hivemind_amd.net import _pack_frag8
    w = (torch.arange(64 * 64) % 251).to(torch.uint8).reshape(64, 64)
    p = _pack_frag8(w)
    assert p.dtype == torch.uint8 and p.numel() == w.numel()
    assert torch.equal(p.sort().values, w.reshape(-1).sort().values)    # a permutation
    # (kstep, tile, lane, j) -> packed index, W row, W column; two tiles, so index = ((kstep/2 * 2 + tile) * 64 + lane) * 16 + (kstep & 1) * 8 + j
    for (ks, tile, lane, j), idx, row, col in (((0, 0, 0, 0), 0, 0, 0), ((3, 1, 37, 5), 3677, 61, 37), ((2, 0, 63, 7), 3063, 47, 31)):
        assert ((ks // 2 * 2 + tile) * 64 + lane) * 16 + (ks & 1) * 8 + j == idx
        assert int(p[idx]) == int(w[row, col]), (ks, tile, lane, j)
