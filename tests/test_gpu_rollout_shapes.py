"""The k_rollout instantiations no default configuration reaches: the eight-wave kernel for the narrow trunk
(HM_ROLLOUT_WAVES8_MIN_ACT) in each of its three search roles, and the four-wave kernel for the 384-channel trunk
(HM_ROLLOUT_WAVES_WIDE=4).  Each case is one single-launch search compared with the lockstep loop of the same engine: root edge
lists, visits, priors, Q, the counters (transposition hits included) must be identical and the hang guard silent.

The kernel choice is read from the environment once per process (function-local statics in hm_sp_search / rollout_kernel), so
every case runs in a child process of its own, started with the variables set: this file run as a script is that child."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one move from mate: the position of the golden case EngineTest.CheckmatePrecedesFiftyMoveDraw before Qxf7#
_MATE_IN_ONE = "r1bqkb1r/pppp1ppp/2n2n2/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - 4 4"
_BARE_KINGS = "4k3/8/8/8/8/8/8/4K3 w - - 0 1"

#        id                 environment                                                  net      slots nodes  mode waves
CASES = {"narrow8_lds":     (dict(HM_ROLLOUT_WAVES8_MIN_ACT="1"),                               "small", 6, 96, 0, 8),
         "narrow8_in_place": (dict(HM_ROLLOUT_WAVES8_MIN_ACT="1", HM_SEARCH_NO_LDS_NODES="1"),  "small", 6, 96, 1, 8),
         "narrow8_shared":  (dict(HM_ROLLOUT_WAVES8_MIN_ACT="1", HM_SEARCH_GAMES_PER_WG="3"),   "small", 6, 96, 2, 8),
         "wide4":           (dict(HM_ROLLOUT_WAVES_WIDE="4"),                                   "full",  3, 64, 2, 4)}


def _roots(G):
    import oracle_py as O
    from test_gpu_search import _transposing_roots
    mate = O.Board()
    mate.set_fen(0, _MATE_IN_ONE)
    mate.set_fen(1, _BARE_KINGS)
    rows = [_transposing_roots()[11:12], mate.compact(0, False)]             # [11]: both boards' kings on move, the richest of the endings at this budget
    rows.append(O.random_positions(900 + G, (G - 2) * 13, 140)[::13][:G - 2])
    return np.concatenate(rows).copy()


def _child(case):
    import torch
    import hivemind_amd as hm
    from hivemind_amd import net as N
    from test_gpu_persistent import _stats_equal
    _, which, G, nodes, _, _ = CASES[case]
    hm.init(0)
    torch.manual_seed(0)
    net = N.FusedNet(N.rise_v3_small() if which == "small" else N.rise_v33())
    roots = _roots(G)
    mask = np.ones(G, np.uint8)
    mask[G - 1] = 0                                                          # an idle slot: its search workgroup (or turn) only signs off
    seeds = (np.arange(G, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(4321)
    eng = hm.SearchEngine(G, nodes + 25)
    assert eng.search_consumers() > 0
    eng.set_games(roots)
    eng.begin_search(nodes, seeds, 0.3, 0.25, mask)
    eng.run(net)
    want = eng.root_stats()
    eng.set_games(roots)
    eng.begin_search(nodes, seeds, 0.3, 0.25, mask)
    assert eng.search_persistent(net) > 0.0
    got = eng.root_stats()
    assert getattr(eng, "stalls", 0) == 0
    _stats_equal(want, got, G)
    info = want["info"]
    for g in range(G):
        assert np.array_equal(info[g, :20], got["info"][g, :20]), (g, info[g], got["info"][g])      # [18]: transposition hits
    print("CHILD tt_hits %s same_batch %s reservation %s statuses %s" % (info[:, 18].tolist(), info[:, 3].tolist(), info[:, 4].tolist(), info[:, 0].tolist()), flush=True)
    if which == "small":
        # the shape is only worth its name if it produced what it was chosen for
        assert int(info[:, 18].sum()) > 0, "no transposition hit"
        assert int(info[:, 3].sum() + info[:, 4].sum()) > 0, "no collision"
    assert int((info[:G - 1, 0] == 3).sum()) >= (G - 1) // 2                 # most live roots really searched (ST_DONE)
    eng.close()
    print("CHILD OK", flush=True)


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_shape_equals_lockstep(hm, case):
    env_add, _, _, _, mode, waves = CASES[case]
    env = dict(os.environ, HM_SEARCH_LOG="1", **env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    lines = [l for l in r.stderr.splitlines() if l.startswith("[hm_sp_search]")]
    assert len(lines) == 1 and f" mode {mode} waves {waves} " in lines[0], lines     # the instantiation under test is the one that ran


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    _child(sys.argv[1])
