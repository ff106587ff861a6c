"""The library's environment switches: one table (csrc/rgl_switches.hip), read through the host-only exports rgl_switch_name /
rgl_switch_parse.  Nothing here needs a GPU, and nothing is read from the environment.

Three parts: every switch parses every text as the rules below say (written out here from the rules each switch had when it had a
reader of its own, not computed from the table); the table's unit is the only place of csrc/ that reads the environment; and the
table and INTEGRATION.md's "Environment switches" section name the same switches.
"""
import ctypes
import glob
import os
import re

import pytest

from relationalgraphlearning_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relationalgraphlearning_amd", "csrc")

TEXTS = (None, "", "0", "1", "2", "10", "-1", "x", "global", "lds")
#                     unset  ""    "0"   "1"   "2"  "10"  "-1"   "x" "global" "lds"
# on only if the first character is 1
ON_IF_1 =            (0,     0,    0,    1,    0,   1,    0,    0,   0,       0)
# on; off only if the first character is 0
OFF_IF_0 =           (1,     1,    0,    1,    1,   1,    1,    1,   1,       1)
# an integer: unset or empty gives the default d, otherwise atoi (0 for text without digits)
def integer(d): return (d,   d,    0,    1,    2,   10,   -1,   0,   0,       0)
# an integer: unset gives -1, anything set -- the empty string too -- goes through atoi
INT_IF_SET =         (-1,    0,    0,    1,    2,   10,   -1,   0,   0,       0)
# unset is on; set: atoi != 0, so empty is off
ON_UNLESS_ZERO =     (1,     0,    0,    1,    1,   1,    1,    0,   0,       0)
# 1 only for exactly "global"
IS_GLOBAL =          (0,     0,    0,    0,    0,   0,    0,    0,   1,       0)

EXPECTED = {
    "RGL_FORCE_GENERIC": ON_IF_1,
    "RGL_CHILDREN_TILE_KERNEL": ON_IF_1,
    "RGL_CHILDREN_FUSED": ON_IF_1,
    "RGL_CHILDREN_TWO_STAGE": ON_IF_1,
    "RGL_REQUIRE_MFMA_CHILDREN": ON_IF_1,
    "RGL_REQUIRE_MFMA_FORWARD": ON_IF_1,
    "RGL_SCENE_WIDE_SLOTS": ON_IF_1,
    "RGL_DEEP_T4": OFF_IF_0,
    "RGL_DEEP_FUSE_HEAD": OFF_IF_0,
    "RGL_SCENE_EMBED_INSIDE": OFF_IF_0,
    "RGL_LEVEL_PROLOGUE": OFF_IF_0,
    "RGL_FUSED_G": integer(0),
    "RGL_FUSED_INLINE_PARTIAL": integer(-1),
    "RGL_FUSED_MIN_TILES": integer(1200),
    "RGL_FUSED_IMAGE_SYNC": integer(0),
    "RGL_FUSED_PHASE_DELAY": integer(0),
    "RGL_FUSED_PRIO": integer(2),
    "RGL_FUSED_HEAD_EARLY": integer(1),
    "RGL_FUSED_NO_TAIL": integer(0),
    "RGL_TILES_FORWARD": integer(1),
    "RGL_BACKWARD_MFMA": integer(-1),
    "RGL_BACKWARD_MFMA_MIN": integer(256),
    "RGL_SARL_GRID_CAP": integer(0),
    "RGL_SCENE_SPLIT_BELOW": INT_IF_SET,
    "RGL_SCENE_CHILDREN_BELOW": INT_IF_SET,
    "RGL_HEAD_ROWS_DIRECT": ON_UNLESS_ZERO,
    "RGL_SARL_PARK": IS_GLOBAL,
}


def table_names():
    lib, names = nat.lib(), []
    while lib.rgl_switch_name(len(names)) is not None:
        names.append(lib.rgl_switch_name(len(names)).decode())
        assert len(names) < 1000
    return names


def test_the_table_holds_the_switches_the_rules_name():
    names = table_names()
    assert len(names) == len(set(names)) and set(names) == set(EXPECTED), set(names) ^ set(EXPECTED)
    assert nat.lib().rgl_switch_name(-1) is None and nat.lib().rgl_switch_name(len(names)) is None


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_parse(name):
    lib, i, v = nat.lib(), table_names().index(name), ctypes.c_int(12345)
    got = []
    for text in TEXTS:
        v.value = 12345
        assert lib.rgl_switch_parse(i, None if text is None else text.encode(), ctypes.byref(v)) == 0, text
        got.append(v.value)
    assert tuple(got) == EXPECTED[name], list(zip(TEXTS, got, EXPECTED[name]))


def test_parse_argument_checks():
    lib, v = nat.lib(), ctypes.c_int(7)
    assert lib.rgl_switch_parse(0, b"1", None) == -3
    assert lib.rgl_switch_parse(-1, b"1", ctypes.byref(v)) == -1 and lib.rgl_switch_parse(len(EXPECTED), b"1", ctypes.byref(v)) == -1
    assert v.value == 7


def test_one_unit_reads_the_environment():
    files = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)]
    assert os.path.join(CSRC, "rgl_switches.hip") in files and len(files) > 40
    for p in files:
        text = open(p, errors="replace").read()
        assert "env_int" not in text, p
        assert ("getenv(" in text) == (os.path.basename(p) == "rgl_switches.hip"), p


def switches_section():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("\n## Environment switches\n", 1)[1]
    return section.split("\n## ", 1)[0]


def test_the_document_names_every_switch_of_the_table():
    documented = set(re.findall(r"RGL_[A-Z0-9_]+", switches_section()))
    assert set(table_names()) <= documented, set(table_names()) - documented


def test_every_documented_switch_exists():
    python = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "relationalgraphlearning_amd", "*.py")) + [os.path.join(ROOT, "bench.py")])
    table = set(table_names())
    for name in set(re.findall(r"RGL_[A-Z0-9_]+", switches_section())):
        assert name in table or re.search(r"\b%s\b" % name, python), name
