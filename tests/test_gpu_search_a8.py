"""The single-launch search with the evaluator on native FP8 MFMA (FusedNet(weights="fp8", acts="fp8", serve=True): hm_net_set_serve,
k_rollout_a8) against the host-driven lockstep loop with the SAME network: the evaluator role rounds every logit once from the fp32
value the stand-alone forward stores, so root statistics and self-play records must be identical bit for bit."""
import numpy as np
import pytest
import torch

import oracle_py as O
from test_gpu_net_a8 import _planes
from test_gpu_persistent import _selfplay, _stats_equal

pytestmark = pytest.mark.gpu

MODELS = {"c128": lambda N: N.RiseV3(128, 160, 32, [3], [True], 8, 256),
          "c128k5": lambda N: N.RiseV3(128, 160, 32, [5, 3], [False, True], 8, 256),
          "c384": lambda N: N.RiseV3(384, 320, 0, [5, 3], [False, True], 16, 512)}


def _fused(hm, name, **kw):
    from hivemind_amd import net as N
    from test_gpu_net import _randomise_bn
    torch.manual_seed(0)
    model = MODELS[name](N)
    _randomise_bn(model, 1)
    return N.FusedNet(model.eval(), weights="fp8", acts="fp8", calibration=_planes(hm, 3), **kw)


# kernel instantiation <CTILES, K5> and search role reached: <4,false> role 0 (enlarged union region) | <4,true> | <12,true> role 2
# (3 games per workgroup, chunked projection) | <12,true> role 0 | role 1 (tree walked in place)
@pytest.mark.parametrize("name,G,cap,nodes,noise,env", [
    ("c128", 12, 200, 120, False, {}),
    ("c128k5", 12, 200, 120, True, {}),
    ("c384", 8, 200, 120, True, {"HM_NET_COP_CHUNK": "192"}),
    ("c384", 8, 200, 120, False, {"HM_SEARCH_GAMES_PER_WG": "1"}),
    ("c128", 6, 1700, 1600, False, {})])
def test_a8_single_launch_search_equals_lockstep(hm, monkeypatch, name, G, cap, nodes, noise, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fused = _fused(hm, name, serve=True)
    roots = O.random_positions(900 + G, G * 13, 140)[::13][:G].copy()
    seeds = (np.arange(G, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(777)
    alpha, eps = (0.3, 0.25) if noise else (0.0, 0.0)
    eng = hm.SearchEngine(G, cap)
    eng.set_games(roots)
    eng.begin_search(nodes, seeds, alpha, eps)
    eng.run(fused)
    want = eng.root_stats()
    for _ in range(2):                                                       # timing differs from run to run; results must not
        eng.set_games(roots)
        eng.begin_search(nodes, seeds, alpha, eps)
        ms = eng.search_persistent(fused)
        assert ms > 0.0 and getattr(eng, "stalls", 0) == 0
        _stats_equal(want, eng.root_stats(), G)
    assert int((want["info"][:, 0] == 3).sum()) >= G // 2                    # most roots really searched (ST_DONE)
    eng.close()


@pytest.mark.parametrize("what", ["serve", "default", "fp16", "w8", "xboard", "cabi_fp16"])
def test_a8_serve_opt_in_and_refusals(hm, what):
    from hivemind_amd import net as N
    from hivemind_amd._lib import lib
    if what in ("serve", "default"):
        fused = _fused(hm, "c128", serve=what == "serve")
        assert fused.serve == (what == "serve") and lib.hm_net_can_serve(fused.handle) == (1 if what == "serve" else 0)
    elif what == "cabi_fp16":
        fused = N.FusedNet(MODELS["c128"](N).eval())
        assert lib.hm_net_set_serve(fused.handle, 1) != 0
    else:
        torch.manual_seed(0)
        model = N.CrossBoardRiseV3(128, 128, 64, [3], [True], 8, 256, attention_layers=1) if what == "xboard" else MODELS["c128"](N)
        with pytest.raises(ValueError):
            N.FusedNet(model.eval(), weights="fp8" if what == "w8" else "fp16", serve=True)


def test_a8_selfplay_takes_the_single_launch(hm, monkeypatch):
    fused = _fused(hm, "c128", serve=True)
    kw = dict(games=16, nodes=100, seed=3, concurrent_games=16, max_macro_plies=60)
    monkeypatch.setenv("HM_SELFPLAY_LOCKSTEP", "1")
    res_l, rec_l, cnt_l = _selfplay(hm, fused, **kw)
    monkeypatch.delenv("HM_SELFPLAY_LOCKSTEP")
    res_p, rec_p, cnt_p = _selfplay(hm, fused, **kw)
    assert res_l.persistent_searches == 0 and res_p.persistent_searches > 0 and res_p.search_kernel_ms > 0
    assert cnt_p == cnt_l and rec_p == rec_l
