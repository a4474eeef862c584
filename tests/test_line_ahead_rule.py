"""Where the 512-thread solve kernel puts a line chunk's records when it evaluates the chunk's pass A under the previous chunk's gather walk
(csrc/uvs_layout.h: uvs_line_ahead_base; csrc/uvs_solve_kernel.h: linearize_roles).  No device: windows are packed by tools/pack_dump, the chunk table is read
out of the blob by tools/line_ahead_rule, and the live ranges of both chunks of every consecutive pair are restated HERE from nob / nlm / nlist and the
constants of uvs_layout.h -- the base the C++ rule returns must intersect none of them and end inside the staging area."""
import os
import subprocess

import pytest

from helpers import uvs
from test_pack_blob import build_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "line_ahead_rule.cpp")
LN_REC, LN_EY, S_DOUBLES = 34, 26, 66 * 16 * 17      # uvs_layout.h: UVS_LN_REC, UVS_LN_EY, UVS_S_DOUBLES

CASES = {      # name -> arguments of synth.make_window
    "benchmark": dict(index=0),
    "benchmark_17": dict(index=17),
    "lines80": dict(index=31, n_lines=80, n_tagged=40, ln_track=5),      # three line chunks of 135 / 135 / 130 observations: the base alternates
    "lines80_full": dict(index=31, n_lines=80, n_tagged=40),             # ... of 189 / 189 / 182 (tracks of 7): each fills the staging area, the rule must refuse
    "ln_track10": dict(index=32, n_lines=44, ln_track=10),               # 150 / 150 / 140 observations: 13 818 + 5 100 doubles do not fit, the rule must refuse
    "ln_track10_40": dict(index=32, ln_track=10),                        # 140 / 130 / 130: fits; the third base is not the first (chunks of unequal size)
    "lines_only": dict(index=33, n_points=0, n_lines=40, n_tagged=30),   # the first line chunk is the first chunk
    "lines8": dict(index=34, n_lines=8, n_tagged=4),                     # one line chunk
    "points_only": dict(index=35, n_lines=0, n_tagged=0),
}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("line_ahead")
    rule = os.path.join(str(d), "line_ahead_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", SRC, "-o", rule])
    return build_driver(d), rule, d


@pytest.fixture(scope="module")
def tables(programs):
    """name -> (pt_rec, pt_xslots, chunks [(type, nob, nlm, nlist)], blob path)"""
    pack, rule, d = programs
    out = {}
    for name, kw in CASES.items():
        w = uvs.synth.make_window(**kw)
        win = os.path.join(str(d), name + ".win"); blob = os.path.join(str(d), name + ".blob")
        w.save(win)
        assert subprocess.check_output([pack, win, blob]).decode().startswith("ok "), name
        rows = [[int(x) for x in ln.split()] for ln in subprocess.check_output([rule, "chunks", blob]).decode().splitlines()]
        pt_rec, xs, n, s_doubles = rows[0]
        assert s_doubles == S_DOUBLES and n == len(rows) - 1
        out[name] = (pt_rec, xs, [tuple(r) for r in rows[1:]], blob)
    return out


def live_ranges(chunk, rec_base, pt_rec, xs):
    """Half-open ranges of staging-area doubles one chunk occupies from its entry barrier to the end of its walk: -> (records, everything else)."""
    t, nob, nlm, nlist = chunk
    lists = (nlist + 1) // 2      # int32 words
    if t == 0:
        assert rec_base == 0
        rec = nob * pt_rec; slots = (nob + xs * nlm) * 6
        return (0, rec), (rec, rec + 2 * slots + lists)      # E | E / h_ll | lists
    rec = nob * LN_REC
    e0 = rec; y0 = e0 + nob * LN_EY; x0 = y0 + nob * LN_EY; l0 = x0 + 20 * nlm      # E | Y | X | lists at the offsets the host's lists name
    return (rec_base, rec_base + rec), (e0, l0 + lists)


def disjoint(a, b):
    return a[1] <= b[0] or b[1] <= a[0] or a[0] == a[1] or b[0] == b[1]


def bases_of(rule, blob):
    return [int(x) for x in subprocess.check_output([rule, "bases", blob]).decode().split()]


def test_records_ahead_touch_nothing_live(programs, tables):
    _, rule, _ = programs
    seen = {}
    for name, (pt_rec, xs, chunks, blob) in tables.items():
        bases = bases_of(rule, blob)
        assert len(bases) == len(chunks) - 1
        rb = 0
        for q, nb in enumerate(bases):
            cur, nxt = chunks[q], chunks[q + 1]
            cur_rec, cur_rest = live_ranges(cur, rb, pt_rec, xs)
            # the chained call and the one-shot call of the rule agree
            one = int(subprocess.check_output([rule, "rule"] + [str(v) for v in (cur_rest[1], rb, cur_rec[1] - cur_rec[0]) + nxt]).decode())
            assert one == nb, (name, q)
            if nxt[0] == 0: assert nb == -1, (name, q)      # point chunks never run ahead
            if nb >= 0:
                mine, nxt_rest = live_ranges(nxt, nb, pt_rec, xs)
                assert nb % 2 == 0 and mine[1] <= S_DOUBLES, (name, q, nb)
                for other in (cur_rec, cur_rest, nxt_rest):
                    assert disjoint(mine, other), (name, q, nb, mine, other)
            rb = nb if nb > 0 else 0
        seen[name] = ([c[0] for c in chunks], bases)
    types, bases = seen["benchmark"]
    assert types == [0, 0, 0, 1, 1] and bases == [-1, -1, 12920, 0]
    assert seen["benchmark_17"][1] == [-1, -1, 12920, 0]
    types, bases = seen["lines80"]
    nl = sum(types)
    assert nl >= 3
    line_bases = [b for t, b in zip(types[1:], bases) if t == 1]
    assert all(b >= 0 for b in line_bases) and all((a > 0) != (b > 0) for a, b in zip(line_bases, line_bases[1:])), line_bases      # high, 0, high, ...
    for name in ("ln_track10", "lines80_full"):
        types, bases = seen[name]
        assert sum(types) >= 3 and any(t == 1 and b == -1 for t, b in zip(types[1:], bases)), (name, types, bases)
    assert seen["ln_track10_40"][1] == [-1, -1, 12904, 0, 11992]
    types, bases = seen["lines_only"]
    assert all(t == 1 for t in types) and len(types) >= 2 and bases[0] > 0
    assert sum(seen["lines8"][0]) == 1
    assert all(b == -1 for b in seen["points_only"][1])


def test_rule_refuses_and_fits_at_the_edges(programs):
    _, rule, _ = programs
    call = lambda *v: int(subprocess.check_output([rule, "rule"] + [str(x) for x in v]).decode())
    nob, nlm, nlist = 140, 20, 958
    end = nob * (LN_REC + 2 * LN_EY) + 20 * nlm + nlist // 2      # 12 919
    assert end == 12919
    assert call(12129, 0, 4000, 1, nob, nlm, nlist) == 12920
    assert call(S_DOUBLES - nob * LN_REC, 0, 4000, 1, nob, nlm, nlist) == S_DOUBLES - nob * LN_REC      # ends exactly at the end of the staging area
    assert call(S_DOUBLES - nob * LN_REC + 1, 0, 4000, 1, nob, nlm, nlist) == -1
    assert call(end, 12920, nob * LN_REC, 1, nob, nlm, nlist) == 0
    assert call(end, 12920, nob * LN_REC, 1, nob + 1, nlm, nlist) == -1      # more records than the current chunk had: they would reach into its E; nothing fits behind either
    assert call(end, 12920, nob * LN_REC, 0, nob, nlm, nlist) == -1
    assert call(12129, 0, 4000, 1, 0, 0, 0) == -1


def test_rule_program_under_sanitizers(programs, tables):
    """The stand-alone program (host code with its own main) under AddressSanitizer and UBSan, once, over every blob."""
    _, _, d = programs
    exe = os.path.join(str(d), "line_ahead_rule_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    for name, (_, _, chunks, blob) in tables.items():
        for mode in ("chunks", "bases"):
            r = subprocess.run([exe, mode, blob], capture_output=True)
            assert r.returncode == 0 and not r.stderr, (name, mode, r.stderr.decode()[-400:])
    r = subprocess.run([exe, "rule", "12129", "0", "4000", "1", "140", "20", "958"], capture_output=True)
    assert r.returncode == 0 and r.stdout.decode().strip() == "12920" and not r.stderr
