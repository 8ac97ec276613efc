"""The rules by which a mesh build simplifies its tape down the octree (fidget_amd/csrc/mesh_split.hpp: where it splits, which cells get
a tape of their own, how the tapes are packed, when a split is used - arithmetic on sizes and paths) built for the host
(tests/host_build/mesh_split_host.cpp) and compared with the same rules restated here.  The bit-exact GPU mesh comparisons pass whenever
a split is skipped: a rule that wrongly turns simplification off shows here, not there.  No GPU.

Line format: `name: key=value ...`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_split_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")


@pytest.fixture(scope="module")
def rules():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "mesh_split_host")
    deps = [SRC, os.path.join(CSRC, "mesh_split.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (plain g++, no HIP headers: the rules touch no device)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, check=True)
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        lines[name] = dict(kv.split("=", 1) for kv in rest.split())
    return lines


def test_split_levels(rules):
    for depth in range(13):
        for n_ops in (255, 256, 6363):
            for n_choices in (0, 5):
                for option in (0, 256):
                    l1 = min(4, depth - 2) if option > 0 and n_ops >= option and n_choices > 0 and depth >= 3 else 0
                    l2 = min(7, depth - 2) if l1 == 4 and depth >= 7 else 0
                    assert rules[f"levels_{depth}_{n_ops}_{n_choices}_{option}"] == {"l1": str(l1), "l2": str(l2)}, (depth, n_ops, n_choices, option)
    # a depth-8 build of prospero.vm splits at 4 and 6, a depth-5 one at 3 alone
    assert rules["levels_8_6363_5_256"] == {"l1": "4", "l2": "6"} and rules["levels_5_6363_5_256"] == {"l1": "3", "l2": "0"}


def expected_pack(level, cands, parent_len, limit):
    """cands: (path, ok, len); candidate j's ops are 1000 * (j + 1) + k.  The rules: accepted where simplification worked and left fewer
    ops than the parent's, and some; table index path - 8^level, dropped at or beyond 8^level; dropped where the ops array would reach
    `limit` entries; offsets in candidate order."""
    n_tab = 8 ** level
    tab, ops, taken = [], [], []
    for j, ((path, ok, n), parent) in enumerate(zip(cands, parent_len)):
        if not (ok and n != 0 and n < parent):
            continue
        idx = path - n_tab
        if idx < 0 or idx >= n_tab or (limit is not None and len(ops) + n >= limit):
            continue
        tab.append((idx, len(ops), n))
        ops += [1000 * (j + 1) + k for k in range(n)]
        taken.append(j)
    join = lambda xs: ",".join(str(x) for x in xs) or "-"
    return {"n_tab": str(n_tab), "tab": join(f"{i}:{o}+{n}" for i, o, n in sorted(tab)), "ops": join(ops), "taken": join(taken), "n_tapes": str(len(taken)),
            "n_ops": str(len(ops))}


@pytest.mark.parametrize("level", [1, 2])
def test_first_split_packing(rules, level):
    b, root = 8 ** level, 10
    cands = [(b + 5, True, 3), (b + 1, False, 4), (b + 2, True, 0), (b + 3, True, root), (b + 4, True, root + 1), (2 * b, True, 2), (b - 1, True, 2), (b + 0, True, 9),
             (b + 6, False, 0), (b + 7, True, 1), (16 * b + 3, True, 2), (b + (63 if level == 2 else 2), True, 4)]
    want = expected_pack(level, cands, [root] * len(cands), None)
    assert rules[f"first_l{level}"] == want
    # ... which is: the four that gained something and lie in the level, in candidate order
    assert want["taken"] == "0,7,9,11" and want["n_tapes"] == "4" and want["n_ops"] == str(3 + 9 + 1 + 4)
    assert want["tab"].startswith("0:3+9,") and want["tab"].endswith(f"{63 if level == 2 else 7}:{12 if level == 1 else 13}+{1 if level == 1 else 4}")


def test_split_worth_using(rules):
    # root tape of 100 ops; kept = sub_ops / (tapes * 100); used below 0.25 for a tape the bulk interpreter would take, below 0.75 for any
    # other; AT the boundary it is not used (the rule says >=); no tapes at all: nothing to use
    for bulk in (0, 1):
        for sub_ops in (0, 99, 100, 101, 299, 300, 301):
            for tapes in (0, 4):
                kept = sub_ops / (tapes * 100) if tapes else 1.0
                assert rules[f"worth_{bulk}_{sub_ops}_{tapes}"] == {"use": str(int(not kept >= (0.25 if bulk else 0.75)))}, (bulk, sub_ops, tapes)
    assert rules["worth_1_99_4"]["use"] == "1" and rules["worth_1_100_4"]["use"] == "0" and rules["worth_1_101_4"]["use"] == "0"
    assert rules["worth_0_299_4"]["use"] == "1" and rules["worth_0_300_4"]["use"] == "0" and rules["worth_0_301_4"]["use"] == "0"


def test_second_split_gate(rules):
    def wanted(in_use, kept, ops, tapes, cells, nch):
        return str(int(in_use and kept > 0 and ops >= 128 * tapes and cells * nch <= 3 << 30))
    assert rules["gate_at"] == {"wanted": wanted(True, 3, 128 * 3, 3, 10, 7)} == {"wanted": "1"}
    assert rules["gate_below"] == {"wanted": wanted(True, 3, 128 * 3 - 1, 3, 10, 7)} == {"wanted": "0"}
    assert rules["gate_unused"] == {"wanted": "0"} and rules["gate_none_kept"] == {"wanted": "0"}
    assert rules["gate_choices_at"] == {"wanted": wanted(True, 3, 1000, 3, 3 << 20, 1024)} == {"wanted": "1"}
    assert rules["gate_choices_over"] == {"wanted": wanted(True, 3, 1000, 3, (3 << 20) + 1, 1024)} == {"wanted": "0"}


def test_second_split_packing(rules):
    # l1 = 1, l2 = 3: the ancestor of a level-3 cell at level 1 is path >> 6, its index in the first split's table (path >> 6) - 8
    sub_of, kept_len = [-1, -1, 0, -1, -1, 1, -1, -1], [8, 6]
    path = lambda a, b, c: (((8 | a) << 3 | b) << 3) | c
    cands = [(path(2, 0, 1), True, 7), (path(3, 1, 1), True, 2), (path(2, 7, 7), True, 8), (path(5, 0, 0), True, 5), (path(5, 0, 1), True, 6), (path(5, 3, 2), False, 2),
             (path(2, 0, 0), True, 1), (path(0, 0, 0), True, 1), (path(7, 7, 7), True, 1), (path(5, 7, 7), True, 0)]
    parents = [sub_of[(p >> 6) - 8] for p, _, _ in cands]
    assert rules["second_parents"] == {"k": ",".join(str(k) for k in parents), "outside": "-1"}
    assert parents == [0, -1, 0, 1, 1, 1, 0, -1, -1, 1]
    want = expected_pack(3, cands, [kept_len[k] if k >= 0 else 0 for k in parents], 1 << 32)
    assert rules["second"] == want
    # a cell whose ancestor kept the root tape (candidates 1, 7, 8) and one as long as its parent (2: 8 of 8, 4: 6 of 6) are skipped
    assert want["taken"] == "0,3,6" and want["n_tab"] == "512"


def test_ops_cap(rules):
    # the second split's ops array stays below 2^32 entries (its table's offsets are 32 bits wide): a candidate that would take it there is
    # dropped, the ones after it still fit; the first split has no limit
    assert rules["cap_pack"] == {"taken": "2", "first": "0", "last": "2", "n_ops": "2"}
    assert rules["cap_fit"] == {"below": "1", "at": "0", "none": "1"}
