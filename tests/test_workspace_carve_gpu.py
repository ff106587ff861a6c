"""The children workspace as the library carves it (carve_children, csrc/rgl_common.h): the weight image slot first, at a place that
depends on neither the parents of a call nor the size the caller passed, then one region its users share.

Every Python caller hands the searches a packed weight image (MprlPlanner.children_image / predictor_image), so the rest of the suite
never runs a search that packs its images into its own workspace.  These tests do, through the raw ABI: the planner TreeSearch
builds, with both images taken away, on a workspace of mprl_tree_workspace_bytes filled with 0xFF bytes -- and require the bits of
the search with the caller's images.  81 actions, depth 2, width 2, clipped; the smallest sizes that reach each branch."""
import ctypes as C

import pytest
import torch

from relationalgraphlearning_amd import _native as nat
from relationalgraphlearning_amd.nets import _stream
from tests.helpers import make_mprl_policy
from tests.test_gpu_parity import seeded_scenes

pytestmark = pytest.mark.gpu
OUTPUTS = ("best_action", "best_value", "root_values", "root_kept")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def searches(dev, mode, H, B):
    """(TreeSearch after a search with the caller's images, its outputs, the same search with no image at hand on an 0xFF workspace)"""
    pol = make_mprl_policy("trained", 2, 2, True, device=dev)
    pol.contraction_dtype = mode
    pol.build_action_space(1.0)
    ts = pol.tree_search()
    robot, humans = seeded_scenes(4000 + H + B, B, H)
    r, h = robot.to(dev), humans.to(dev)
    with torch.no_grad():
        want = {k: v.clone() for k, v in ts.search(r, h, True).items()}
    lib = nat.lib()
    with torch.cuda.device(dev):
        pl = ts.planner(dev)
        pl.children_image, pl.predictor_image = None, None
        nbytes = lib.mprl_tree_workspace_bytes(C.byref(pl), B, H)
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        got = {"best_action": torch.empty(B, dtype=torch.int32, device=dev), "best_value": torch.empty(B, device=dev),
               "root_values": torch.empty(B, 2, device=dev), "root_kept": torch.empty(B, 2, dtype=torch.int32, device=dev)}
        nat.check(lib.mprl_tree_search_f32(C.byref(pl), r.data_ptr(), h.data_ptr(), B, H, 1, ws.data_ptr(), nbytes,
                                           got["best_action"].data_ptr(), got["best_value"].data_ptr(), got["root_values"].data_ptr(),
                                           got["root_kept"].data_ptr(), _stream()), "mprl_tree_search_f32")
        torch.cuda.synchronize(dev)
    return ts, want, got


# f32, H = 19, B = 128: level 0 (128 parents, 768 tiles: under RGL_FUSED_MIN_TILES) runs the two-stage pair on the image the search
#   packed for its 256 widest parents, level 1 the fused kernel on the same slot -- a smaller P finds the image packed for the larger
# f32, H = 19, B = 3: no level reaches the fused kernel, no image is packed: the pair builds its weights from the raw matrices
# bf16x6, H = 19, B = 3: the fused bf16 form at any P; the partial tile's rows (81 mod 16 = 1) and the image share one workspace
# bf16x6, H = 24, B = 128: level 1 is an own_image call -- the f32 form on an f32 image the call packs into the slot itself
# f32, H = 40, B = 3: H + 1 > 32, no image slot: the stage-1 rows start the region, which starts the workspace
@pytest.mark.parametrize("mode,H,B", [("f32", 19, 128), ("f32", 19, 3), ("bf16x6", 19, 3), ("bf16x6", 24, 128), ("f32", 40, 3)])
def test_search_that_packs_its_own_images_matches_the_callers_images(mode, H, B, dev):
    _, want, got = searches(dev, mode, H, B)
    for k in OUTPUTS:
        assert torch.equal(got[k], want[k]), (mode, H, B, k)


def test_one_children_workspace_serves_calls_of_fewer_parents(dev):
    """mprl_value_children_f32 on the level-1 inputs of the first case, with ONE workspace sized for 256 parents: at P = 256 (the fused
    kernel) and then at P = 128 (the two-stage pair), each packing or building its own weights, against the same call with the
    caller's children_image -- how a benchmark's hand-off buffer is used."""
    ts, _, _ = searches(dev, "f32", 19, 128)
    lv = ts.level_arrays(1)
    child_robot, humans_next = lv["child_robot"].clone(), lv["humans_next"].clone()
    assert child_robot.shape[0] == 256
    lib = nat.lib()
    with torch.cuda.device(dev):
        pl = ts.planner(dev)
        nbytes = lib.mprl_value_children_workspace_bytes(C.byref(pl), 256, 19)
        bare = ts.planner(dev)
        bare.children_image = None
        assert nbytes > 0 and lib.mprl_value_children_workspace_bytes(C.byref(bare), 256, 19) == nbytes
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        for P in (256, 128):
            out = []
            for planner in (pl, bare):
                v = torch.empty(P, 81, device=dev)
                nat.check(lib.mprl_value_children_f32(C.byref(planner), child_robot.data_ptr(), humans_next.data_ptr(), P, 19,
                                                      v.data_ptr(), ws.data_ptr(), nbytes, _stream()), "mprl_value_children_f32")
                out.append(v)
            torch.cuda.synchronize(dev)
            assert torch.equal(out[0], out[1]), P
