"""CPU half of the level prologue's cooperative-embedding tests (-m "not gpu"): the case table of tests/prologue_embedding.py, held
against the library's own planner (rgl_plan_prologue_embedding: host only).  Each condition fails when the search that meets it is
taken out of the table."""
import ctypes

from relationalgraphlearning_amd import _native as nat
from tests import prologue_embedding as pe

ROW_BUFFER_BYTES = 163728 - 131136          # what lies free behind the prologue's scene region in the kernel's dynamic LDS


def all_levels():
    for case in pe.CASES:
        for l, P, cp, unit in pe.levels(case):
            yield case, l, pe.plan(case, l)


def folded():
    return [(case, l, p) for case, l, p in all_levels() if p["prologue"]]


def test_every_level_at_or_above_the_threshold_takes_the_prologue():
    n = 0
    for case, l, p in all_levels():
        above = -(-p["P"] // pe.CUS) >= pe.MIN_PARENTS_PER_CU
        assert p["prologue"] == int(above), (case, l, p)
        n += above
    assert n == 15 and all(any(p["prologue"] for c, _, p in all_levels() if c == case) for case in pe.CASES)


def test_the_plan_is_consistent_and_the_row_buffer_fits():
    for case, l, p in folded():
        k, cp, H = p["parents_per_wg"], p["crowds_per"], p["H"]
        assert p["workgroups"] == -(-p["P"] // k) <= pe.CUS and k % p["unit"] == 0, (case, l, p)
        assert p["chunk_crowds"] == 12 and p["row_floats"] == (12 * H + 16) * 32 and 4 * p["row_floats"] <= ROW_BUFFER_BYTES, (case, l, p)
        ch = pe.chunks(p, 0, k)
        assert len(ch) == p["chunks_per_wg"] and ch[0][1] == p["chunk_parents"] <= 16, (case, l, p, ch)
        crowds0 = (ch[0][1] - 1) // cp + 1
        assert p["human_tiles"] == -(-crowds0 * H // 16) and p["robot_tiles"] == 1, (case, l, p)
        for b in range(p["workgroups"]):                     # every chunk of every workgroup stays inside the buffer
            for c0, c1 in pe.chunks(p, b * k, min((b + 1) * k, p["P"])):
                assert 1 <= c1 - c0 <= 16 and (c1 - 1) // cp - c0 // cp + 1 <= p["chunk_crowds"], (case, l, b, c0, c1)


def test_the_table_holds_a_case_of_each_kind():
    f = folded()
    # a crowd split by a workgroup boundary: sibling parents of one crowd on two workgroups
    assert any(p["crowds_per"] > 1 and p["parents_per_wg"] % p["crowds_per"] for _, _, p in f)
    # a workgroup with more than one chunk -- by the parent bound and by the crowd bound
    assert any(p["chunks_per_wg"] > 1 and p["crowds_per"] > 1 for _, _, p in f)
    assert any(p["chunks_per_wg"] > 1 and p["crowds_per"] == 1 and p["chunk_parents"] == 12 for _, _, p in f)
    # a short last workgroup
    assert any(p["P"] % p["parents_per_wg"] for _, _, p in f)
    # N = 17, and a human tile that spans two crowds
    assert any(p["H"] == 16 for _, _, p in f)
    assert any(p["H"] % 16 and (p["chunk_parents"] - 1) // p["crowds_per"] >= 1 for _, _, p in f)
    # a chunk that starts inside a crowd (its siblings' rows are embedded on both sides of the boundary)
    assert any(c0 % p["crowds_per"] for _, _, p in f for c0, _ in pe.chunks(p, 0, p["parents_per_wg"]))


def test_levels_outside_the_form_keep_their_three_launches_and_bad_arguments_are_refused():
    lib, p = nat.lib(), nat.RglPrologueEmbeddingPlan()
    ref = ctypes.byref

    def ask(pl, P=4096, H=19, cp=2, unit=1):
        assert lib.rgl_plan_prologue_embedding(ref(pl), P, H, cp, unit, ref(p)) == 0
        return p.prologue

    assert ask(pe.planner(2, 2)) == 1
    assert ask(pe.planner(2, 2), P=512) == 0 and (p.parents_per_wg, p.row_floats) == (0, 0)      # 2 parents per CU
    assert ask(pe.planner(2, 2), H=15) == 0 and ask(pe.planner(2, 2), H=20) == 0                 # one node tile; 21 nodes
    pl = pe.planner(2, 2)
    pl.contraction_dtype = nat.CONTRACTION_DTYPES["f32"]
    assert ask(pl) == 0
    pl = pe.planner(2, 2)
    pl.linear_state_predictor = 1
    assert ask(pl) == 0
    pl = pe.planner(2, 2)
    pl.predictor_graph.num_layer = 4                       # a deeper predictor's image leaves room for fewer crowds per chunk
    assert ask(pl) == 1 and 1 <= p.chunk_crowds < 12 and p.row_floats == (p.chunk_crowds * 19 + 16) * 32
    pl = pe.planner(2, 2)
    assert lib.rgl_plan_prologue_embedding(None, 4096, 19, 2, 1, ref(p)) == -3
    assert lib.rgl_plan_prologue_embedding(ref(pl), 4096, 19, 2, 1, None) == -3
    for P, H, cp, unit in ((0, 19, 2, 1), (4096, 0, 2, 1), (4096, 19, 0, 1), (4096, 19, 2, 0), (4097, 19, 2, 1)):
        assert lib.rgl_plan_prologue_embedding(ref(pl), P, H, cp, unit, ref(p)) == -1, (P, H, cp, unit)
