"""The ground the device exploration stands on, checked without a GPU: the restatement of the exploration stream
(tests/explore_cpu.py, which csrc/rgl_explore.hip is written from) against numpy itself, the host generator's draw count against
the scene restatement's, the two entry points' host-side argument checks, VectorExplorer's refusals, and the reference fixture
tests/golden/explore.npz against the restatement."""
import ctypes
import types

import numpy as np
import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd import sim as simmod
from relationalgraphlearning_amd.sim import BASE_SEED, SimConfig
from relationalgraphlearning_amd.vector_explorer import VectorExplorer
from tests import explore_cpu as xc
from tests import golden_io as gio
from tests import scenegen_cpu as sg

T = 200
N_ACTIONS = (1, 2, 81, 128, 129, 256)
EPSILONS = (0.0, 0.3, 1.0)
# Where the first decision starts.  Scene generation takes doubles, two words each, so by itself it leaves an even position;
# an odd one is reached through an exploring decision of three words (n = 2, epsilon = 1: its mask is 1, nothing is rejected).
# (name, doubles, whether that preliminary decision is made): 624 = a fresh seed, 0 = one whole block of 624 words spent (the
# state's position is 624 again, one twist later), 621 so that a choice's first draw is the last word of a block.
STARTS = (("622", 311, False), ("623", 310, True), ("624", 0, False), ("0", 312, False), ("621", 309, True))
SEEDS = (2000, 2001, 2002, 2003, 2 ** 32 - 2)


def _numpy_decisions(seed, doubles, preliminary, n, epsilon, greedy):
    saved = np.random.get_state()
    try:
        np.random.seed(seed)
        for _ in range(doubles):
            np.random.random_sample()
        if preliminary:
            assert np.random.random() < 1.0
            np.random.choice(2)
        out = []
        for g in greedy:
            probability = np.random.random()
            if probability < epsilon:
                out.append((int(np.random.choice(n)), 1))
            else:
                out.append((int(g), 0))
        return out, np.random.get_state()
    finally:
        np.random.set_state(saved)


def test_restatement_equals_numpy_and_the_cases_meet_every_twist():
    met = {"twist_inside_random": 0, "twist_before_choice": 0, "twist_in_rejection": 0, "rejections": 0, "twists": 0}
    n_cases = 0
    for name, doubles, preliminary in STARTS:
        for seed in SEEDS:
            for n in N_ACTIONS:
                for epsilon in EPSILONS:
                    greedy = [(7 * t + seed) % n for t in range(T)]
                    want, state = _numpy_decisions(seed, doubles, preliminary, n, epsilon, greedy)
                    key, pos = state[1], state[2]
                    st = xc.ExploreStream(seed, doubles)
                    if preliminary:
                        st.decide(0, 2, 1.0)
                    start = int(st.words()[624])
                    assert start == (int(name) if name != "0" else 624), (name, start)
                    got = [st.decide(g, n, epsilon) for g in greedy]
                    assert got == want, (name, seed, n, epsilon)
                    words = st.words()
                    assert words.shape == (xc.STATE_WORDS,) and int(words[624]) == pos, (name, seed, n, epsilon)
                    assert np.array_equal(words[:624], key), (name, seed, n, epsilon)       # the draw that follows is aligned too
                    for k in met:
                        met[k] += getattr(st, k)
                    n_cases += 1
    print("%d cases of %d decisions: %s" % (n_cases, T, met))
    assert met["twist_inside_random"] >= 1, "no case twists between the two words of random()"
    assert met["twist_before_choice"] >= 1, "no case twists between random() and the choice"
    assert met["twist_in_rejection"] >= 1, "no case twists inside a rejection loop"
    assert met["rejections"] >= 1, "no case rejects a draw"


def test_seeded_state_is_the_stream_after_the_scenes_doubles():
    for seed in (0, 2000, 2 ** 32 - 1):
        for d in (0, 1, 311, 312, 313, 935, -3):
            rs = np.random.RandomState(seed)
            rs.random_sample(max(d, 0))
            _, key, pos = rs.get_state()[:3]
            words = xc.ExploreStream(seed, d).words()
            assert np.array_equal(words[:624], key) and int(words[624]) == pos, (seed, d)
    assert xc.draws_for_position(622) == 311 and xc.draws_for_position(0) == 312 and xc.draws_for_position(2, twists=2) == 313


@pytest.mark.parametrize("scenario,human_num", [("circle_crossing", 5), ("square_crossing", 4)])
@pytest.mark.parametrize("randomize", [False, True])
def test_host_generator_counts_the_draws_it_takes(scenario, human_num, randomize):
    cfg = SimConfig(scenario=scenario, human_num=human_num, randomize_attributes=randomize)
    for phase, case in (("train", 0), ("train", 1), ("train", 7), ("val", 3), ("test", 11), ("train", sg.TRAIN_SIZE - 1)):
        plain = simmod.generate_scene(cfg, phase, case)
        counted = simmod.generate_scene_with_draws(cfg, phase, case)
        restated = sg.generate_scene_restated(cfg, phase, case)
        assert len(plain) == 4 and len(counted) == 5
        assert all(np.array_equal(a, b) for a, b in zip(plain, counted[:4]))
        assert counted[4] == restated[4]["draws"] == sg.host_scene_with_draws(cfg, phase, case)[4], (phase, case)


def test_entry_points_are_exported_and_check_their_arguments_on_the_host():
    lib = nat.lib()
    for name in ("crowd_explore_seed_u32", "crowd_explore_select_f64"):
        assert name in nat.SIGNATURES and name in nat.ADDITIVE
    assert nat.EXPLORE_STATE_WORDS == xc.STATE_WORDS == 625
    p = ctypes.c_void_p(16)                      # never dereferenced: every call below is refused before a launch
    assert lib.crowd_explore_seed_u32(None, p, 1, p, None) == -3
    assert lib.crowd_explore_seed_u32(p, None, 1, p, None) == -3
    assert lib.crowd_explore_seed_u32(p, p, 1, None, None) == -3
    assert lib.crowd_explore_seed_u32(p, p, 0, p, None) == -1

    def call(epsilon=0.5, B=1, n_actions=81, **missing):
        job = nat.CrowdExploreJob()
        for field in ("greedy", "done", "table", "state", "chosen", "action", "explored"):
            setattr(job, field, None if field in missing else 16)
        job.epsilon, job.B, job.n_actions = epsilon, B, n_actions
        return lib.crowd_explore_select_f64(ctypes.byref(job))
    assert lib.crowd_explore_select_f64(None) == -3
    for field in ("greedy", "done", "table", "state", "chosen", "action"):
        assert call(**{field: True}) == -3, field
    assert call(B=0) == -1 and call(n_actions=0) == -1 and call(n_actions=nat.MAX_ACTIONS + 1) == -1
    assert call(epsilon=float("nan")) == -2 and call(epsilon=-1e-9) == -2 and call(epsilon=1.0 + 1e-9) == -2
    assert call(epsilon=float("nan"), explored=True) == -2          # `explored` may be absent: the call gets as far as epsilon


class _Policy(object):
    name, epsilon, action_space = "stub", 0.5, None

    def set_phase(self, phase):
        self.phase = phase

    def build_action_space(self, v_pref):
        self.action_space = [(0.0, 0.0), (1.0, 0.0)]


class _LoadedSim(object):
    """A simulator whose reset loads states from elsewhere: no seeds, no draw counts."""
    device, cfg, kinematics, B = torch.device("cpu"), SimConfig(), "holonomic", 2
    scene_seeds = scene_draws = None
    done = torch.zeros(2, dtype=torch.int32)

    def reset(self, phase, cases):
        return torch.zeros(2, 9), torch.zeros(2, 5, 5)


def test_vector_explorer_refuses_an_unknown_mode_and_states_without_seeds():
    with pytest.raises(ValueError, match="exploration"):
        VectorExplorer(_LoadedSim(), _Policy(), exploration="numpy")
    assert VectorExplorer(_LoadedSim(), _Policy()).exploration == "host"
    ex = VectorExplorer(_LoadedSim(), _Policy(), exploration="device")
    with pytest.raises(ValueError, match="seeded"):
        ex.run_k_episodes(2, "train")


def test_reference_fixture_follows_from_the_restatement():
    """tests/golden/explore.npz (the reference Explorer exploring, make_golden_explore.py): every decision's probability,
    explored flag and index is what the restatement gives for the case's seed and draw count."""
    fx = gio.load("explore")
    cases, n, epsilon = fx["ex.cases"], int(fx["ex.n_actions"]), float(fx["ex.epsilon"])
    cfg = SimConfig(circle_radius=float(fx["ex.circle_radius"]), time_limit=float(fx["ex.time_limit"]))
    ends = fx["ex.steps_end"]
    actions, probability, choice = (np.split(fx["ex." + k], ends[:-1]) for k in ("actions", "probability", "choice"))
    assert len(cases) == 8 == len(actions) and n == 81 and 0.0 < epsilon < 1.0
    explored = rejections = 0
    for i, case in enumerate(cases):
        draws = simmod.generate_scene_with_draws(cfg, "train", int(case))[4]
        assert draws == int(fx["ex.draws"][i])
        st = xc.ExploreStream(BASE_SEED["train"] + int(case), draws)
        for a, p, c in zip(actions[i], probability[i], choice[i]):
            chosen, took = st.decide(int(a), n, epsilon)
            assert st.last_u == float(p) and took == int(c >= 0) and chosen == int(a) and (c < 0 or c == a), (case, a, p, c)
            explored += took
        rejections += st.rejections
    assert explored >= 10 and rejections >= 1, (explored, rejections)
    assert float(fx["ex.min_gap"]) >= 1e-4
