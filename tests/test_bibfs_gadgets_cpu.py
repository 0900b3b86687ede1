"""helpers.bibfs_gadgets and tests/bibfs_model.py, without a GPU: the model equals the oracle's BFS wherever it answers, every
gadget is what it claims to be (on the model's trace, not on the builder's bookkeeping), every mutant of the model is told
apart by a named family, and helpers.BIBFS_LIMITS is what the sources say.  test_bibfs_limits_gpu.py runs the same rows on
the device."""
import os
import re

import numpy as np
import pytest

import bibfs_model as M
from helpers import (BIBFS_FAR, BIBFS_HUB, BIBFS_LENGTHS, BIBFS_LIMITS, BIBFS_POSITIONS, BIBFS_SHIPPED_CAP, BIBFS_TEST_CAP, BIBFS_TIES,
                     bibfs_calls, bibfs_gadgets, bibfs_stale_gadgets)
from oracle.pgq_oracle import OracleCSR

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "duckpgq-extension_amd", "csrc")
GRID = 256  # the MI355X's CUs; the layout argument of the stale family holds for any grid below qcap - 4


class Side:
    def __init__(self, g):
        self.g = g
        ora = OracleCSR.from_edges(g.V, g.src, g.dst)
        ln, ok = ora.lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        self.mg = M.Graph(g.V, g.src, g.dst)
        self.calls = {name: (fam, q, cap, rows, M.solve(self.mg, (g.rs[rows], g.rd[rows]), cap, q)) for name, fam, q, cap, rows in bibfs_calls(g)}

    def solve(self, rows, cap=BIBFS_SHIPPED_CAP, q=1024, **kw):
        return M.solve(self.mg, (self.g.rs[rows], self.g.rd[rows]), cap, q, **kw)


@pytest.fixture(scope="module")
def sides():
    g = bibfs_gadgets()
    return [Side(g), Side(g.transposed())]


def answers(res):
    return np.array([r.answer for r in res])


# ---- the model is the oracle's BFS wherever it answers ---------------------------------------------------------------------
def test_model_equals_oracle_on_the_gadgets(sides):
    n = {}
    for k, side in enumerate(sides):
        g = side.g
        assert g.V < 150_000 and (side.dist == g.dist).all()
        for name, (fam, q, cap, rows, res) in side.calls.items():
            ans = answers(res)
            opn = ans == M.OPEN
            assert (ans[~opn] == side.dist[rows][~opn]).all(), name
            # open: the level of qcap + 1, the work of cap + 1, and the decoy rows behind a list of 1025 (a level of 1025 vertices)
            want_open = {"queue_1024": 1, "queue_2048": 1, "cap": 1, "slots": 4}.get(name, 0)
            assert opn.sum() == want_open, (name, int(opn.sum()))
            n[name] = len(rows)
    print("rows per call:", n)
    assert n["slots"] == sum(BIBFS_LENGTHS) * 4 + 257 + 4 * len(BIBFS_LENGTHS) + 1 and n["slots"] < 17_000
    assert n["positions_1024"] == sum(BIBFS_POSITIONS[1024]) + 1024 and n["positions_2048"] == sum(BIBFS_POSITIONS[2048])


def test_model_equals_oracle_on_random_graphs_under_caps_and_bounds():
    rng = np.random.default_rng(11)
    seen_open = seen_null = 0
    for trial in range(40):
        V = int(rng.integers(4, 120))
        E = int(rng.integers(V // 2, V * 5))
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        ps, pd = rng.integers(0, V, 60), rng.integers(0, V, 60)
        ln, ok = OracleCSR.from_edges(V, s, d).lean_iterativelength(V, ps, pd)
        dist = np.where(ok, ln, -1)
        g = M.Graph(V, s, d)
        for cap, q, bound in ((1 << 30, 1 << 30, None), (12, 1 << 30, None), (1 << 30, 6, None), (1 << 30, 1 << 30, 3), (12, 6, 4)):
            for gm in (False, True):
                ans = answers(M.solve(g, (ps, pd), cap, q, bound=bound, grid=3 if gm else None, gm=gm))
                want = dist if bound is None else np.where(dist > bound, -1, dist)
                opn = ans == M.OPEN
                assert (ans[~opn] == want[~opn]).all(), (trial, cap, q, bound, gm)
                assert cap < 1 << 30 or q < 1 << 30 or not opn.any()
                seen_open += int(opn.sum())
                seen_null += int((ans == M.NULL).sum())
    assert seen_open > 100 and seen_null > 100


# ---- every gadget is what it claims to be ----------------------------------------------------------------------------------
def test_positions_every_queue_position_has_a_row_of_its_own(sides):
    for k, side in enumerate(sides):
        g = side.g
        for name in ("positions_1024", "positions_2048"):
            fam, q, cap, rows, res = side.calls[name]
            for a in np.unique(g.a[rows]):
                F = int(a) & 0xFFFFF
                sel = np.flatnonzero(g.a[rows] == a)
                assert len(sel) == F
                wit = []
                for i in sel:
                    r = res[i]
                    if r.answer == M.NULL:  # a dead end's row
                        assert a >> 20 and int(g.b[rows[i]]) % 3 == 1
                        continue
                    side_, nf, work, new, hits = r.levels[-1]
                    # the walk over the F queue positions of the source's side met the other side, at one adjacency entry
                    assert (r.answer, side_, nf, len(hits)) == (3, k, F, 1), (name, F, i)
                    wit.append(int(hits[0]))
                live = F if not a >> 20 else F - len(range(1, F, 3))
                assert len(set(wit)) == len(wit) == live, (name, F)  # one entry, so one queue position, per row
        assert {int(a) for a in np.unique(g.a[g.rows_where("positions")])} == \
            set(BIBFS_POSITIONS[1024]) | set(BIBFS_POSITIONS[2048]) | {1024 + (1 << 20)}
    L = BIBFS_LIMITS
    per_pass = L["walk_stride"] * L["walk_lanes"]
    assert per_pass == L["block"] == L["queue_floor"]
    for lim in (L["walk_stride"], per_pass - L["walk_stride"], per_pass, 2 * per_pass):  # a wavefront's last lane, the last pass
        assert {lim - 1, lim, lim + 1} - {2 * per_pass + 1} <= set(BIBFS_POSITIONS[1024]) | set(BIBFS_POSITIONS[2048]), lim


def test_slots_every_list_slot_has_a_row_of_its_own(sides):
    L = BIBFS_LIMITS
    for lim in (L["chunk"], 2 * L["chunk"]):
        assert {lim - 1, lim, lim + 1} <= set(BIBFS_LENGTHS)
    assert L["depth"] * L["chunk"] + 1 <= 769 and 4 * L["chunk"] + 1 == 1025  # the refill after DEPTH chunks; a fifth chunk
    for k, side in enumerate(sides):
        g = side.g
        fam, q, cap, rows, res = side.calls["slots"]
        xoff = side.mg.xoff[k]
        assert {(n, kk) for n, kk, f, last in g.slots} >= {(n, kk) for n in BIBFS_LENGTHS for kk in range(4)}
        for n, (Ln, kk, f, last) in enumerate(g.slots):
            b, e = int(xoff[f]), int(xoff[f + 1])
            assert e - b == Ln and b % 4 == kk, (n, Ln, kk, b)
            assert (e == side.mg.E) == last
            sel = np.flatnonzero(g.a[rows] == n)
            slots = []
            for i in sel:
                r = res[i]
                if g.b[rows[i]] < 0:  # the decoy row: the pad's and the upper neighbour's entries are its destination, and only theirs
                    assert r.answer == (M.OPEN if Ln > q else M.NULL), (n, Ln)
                    adj = side.mg.xadj[k]
                    d = g.rd[rows[i]] if k == 0 else g.rs[rows[i]]
                    assert (adj[b - kk:b] == d).all() and (last or (adj[e:e + 3] == d).all()) and not (adj[b:e] == d).any()
                    continue
                assert r.answer == 3
                hits = r.levels[-1][4]
                assert len(hits) == 1
                if Ln >= 3:  # met inside f's list; shorter lists: one level later, by the vertex the slot queued
                    walked = [lv for lv in r.levels if lv[0] == k and lv[1] == 1 and lv[2] == Ln]  # the source's side walks f's list, alone
                    assert len(walked) == 1 and walked[0] is r.levels[-1] and b <= hits[0] < e, (n, Ln)
                    slots.append(int(hits[0]) - b)
            assert Ln < 3 or sorted(slots) == list(range(Ln)), (n, Ln)
        assert sum(last for *_, last in g.slots) == 1


def test_queue_cap_tie_and_far_sit_on_the_constants(sides):
    for k, side in enumerate(sides):
        g = side.g
        for q in (1024, 2048):
            fam, _, cap, rows, res = side.calls["queue_%d" % q]
            for i, r in enumerate(res):
                Q = int(g.a[rows[i]])
                assert r.levels[1][:4] == (k, 1, Q, Q)  # the source's Q out-entries, Q new vertices
                assert (r.answer, len(r.levels)) == ((6, 6) if Q == q else (M.OPEN, 2)), (q, Q)
            assert sorted(g.a[rows].tolist()) == [q, q + 1]
        fam, q, cap, rows, res = side.calls["cap"]
        assert cap == BIBFS_TEST_CAP and sorted(g.a[rows].tolist()) == [cap, cap + 1] and BIBFS_HUB > 2049
        for U in (None, 6, 7, 8, 9):
            for i, r in enumerate(side.solve(rows, cap, q, bound=U)):
                C = int(g.a[rows[i]])
                assert len(r.sides) >= 6 and r.sides[:6] == (k,) * 5 + (k ^ 1,)  # a + b = 6 when the side of work C is chosen
                want = M.NULL if U == 6 else M.OPEN if C > cap else 8 if U is None or U >= 8 else M.NULL
                assert r.answer == want, (U, C, r.answer)
                if U != 6 and C == cap:
                    assert r.levels[6][:3] == (k, 1, C)
        fam, q, cap, rows, res = side.calls["tie"]
        for i, r in enumerate(res):
            t = int(g.a[rows[i]])
            assert r.levels[0][2] == t and r.answer == M.NULL and r.sides == (0,) * len(r.sides)  # equal work: forward
            assert r.entries == (2 * t if k == 0 else t)
            back = side.solve(rows[i:i + 1], mutant="tie_backward")[0]
            assert back.entries == (t if k == 0 else 2 * t) and back.sides == (1,) * len(back.sides)
        assert sorted(g.a[rows].tolist()) == list(BIBFS_TIES)
        fam, q, cap, rows, res = side.calls["far"]
        d = side.dist[rows]
        assert set(d[g.b[rows] == 0].tolist()) == set(BIBFS_FAR) and (d[g.b[rows] % 2 == 1] == -1).all() and min(BIBFS_FAR) == 5


def test_stale_rows_list_what_they_claim():
    g0, Ts = bibfs_stale_gadgets(GRID)
    assert g0.V < 150_000 and sorted(Ts) == [1023, 1024, 1025]
    for k, g in enumerate((g0, g0.transposed())):
        ln, ok = OracleCSR.from_edges(g.V, g.src, g.dst).lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
        mg = M.Graph(g.V, g.src, g.dst)
        res = M.solve(mg, (g.rs, g.rd), BIBFS_SHIPPED_CAP, 1024, grid=GRID, gm=True)
        assert (answers(res) == np.where(ok, ln, -1)).all() and (np.where(ok, ln, -1) == g.dist).all()
        for i, r in enumerate(res):
            if g.b[i] == 0:  # dirty: the source's side marks T vertices, one per word, and lists what the row claims
                assert r.listed == g.a[i] and r.levels[0][:4] == (k, 1, Ts[int(g.a[i])], Ts[int(g.a[i])]) and r.sides == (k,) * 3
                c = (g.dst if k == 0 else g.src)[(g.src if k == 0 else g.dst) == (g.rs if k == 0 else g.rd)[i]]
                assert len(np.unique(c >> 5)) == len(c) == Ts[int(g.a[i])]
            elif g.b[i] == 1:  # the destination's side is the cheaper one and reaches every one of the T vertices
                assert r.answer == M.NULL and r.levels[0][:4] == (k ^ 1, 1, Ts[int(g.a[i])], Ts[int(g.a[i])])
            else:
                assert r.answer == 2 and r.sides == (k, k)
        # workgroup w: dirty, victim, dirty, victim of the second kind, for each of the three list lengths
        assert g.b.reshape(-1, GRID).tolist() == [[x] * GRID for x in (0, 1, 0, 2) * 3]


# ---- every mutant is told apart, by the family named here ------------------------------------------------------------------
def pick(side, name, keep):
    fam, q, cap, rows, res = side.calls[name]
    sel = np.array([i for i in range(len(rows)) if keep(int(side.g.a[rows[i]]), int(side.g.b[rows[i]]))], dtype=np.int64)
    return rows[sel], [res[i] for i in sel], cap, q


slot_gadget = lambda L: (lambda a, b: a in [4 * BIBFS_LENGTHS.index(L) + kk for kk in range(4)])
KILLS = {  # mutant: (call, rows of it, bound, what differs)
    "cap_ge": ("cap", lambda a, b: True, None, "answer"),
    "queue_ge": ("queue_1024", lambda a, b: True, None, "answer"),
    "queue_drop_last": ("positions_1024", lambda a, b: a == 1024, None, "answer"),
    "second_pass_lost": ("positions_2048", lambda a, b: a == 1025, None, "answer"),
    "cnt_floor": ("positions_1024", lambda a, b: a == 17, None, "answer"),
    "head_unmasked": ("slots", slot_gadget(5), None, "answer"),
    "tail_unmasked": ("slots", slot_gadget(5), None, "answer"),
    "second_chunk_lost": ("slots", slot_gadget(257), None, "answer"),
    "third_chunk_lost": ("slots", slot_gadget(513), None, "answer"),
    "empty_list_stops": ("positions_1024", lambda a, b: a == 1024 + (1 << 20), None, "answer"),
    "bound_after_cap": ("cap", lambda a, b: True, 6, "answer"),
    "bound_ge_plus_1": ("cap", lambda a, b: True, 6, "answer"),
    "tie_backward": ("tie", lambda a, b: True, None, "entries"),  # no path either way: the entry count tells which side ran
}
STALE_KILLS = {"stale_own": 0, "stale_other": 1, "overflow_list_clear": 0, "first_row_trusts_map": 0}  # mutant: orientation


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_every_mutant_is_told_apart(sides, mutant):
    assert set(KILLS) | set(STALE_KILLS) == set(M.MUTANTS)
    if mutant in STALE_KILLS:
        grid = 32  # the rows of a workgroup follow each other as they do under GRID: fewer workgroups tell the same
        g, _ = bibfs_stale_gadgets(grid)
        g = g.transposed() if STALE_KILLS[mutant] else g
        mg = M.Graph(g.V, g.src, g.dst)
        base, res = (M.solve(mg, (g.rs, g.rd), BIBFS_SHIPPED_CAP, 1024, grid=grid, gm=True, mutant=m) for m in (None, mutant))
        diff = np.flatnonzero(answers(base) != answers(res))
        assert len(diff), mutant
        got = {(int(g.a[i]), int(g.b[i]), int(answers(res)[i])) for i in diff}
        if mutant.startswith("stale"):  # a false meeting behind every dirty row, a dropped vertex behind every dirty row
            assert got >= {(n, 1, 1) for n in (1023, 1024)} | {(n, 2, M.NULL) for n in (1023, 1024)}, got
        if mutant == "overflow_list_clear":  # only behind a list of qcap + 1 words (the first victim lists as many as its dirty row)
            assert (1025, 1, 1) in got and {n for n, _, _ in got} == {1025}, got
        # without the global maps' state there is nothing to tell: every row starts on a cleared map
        again = M.solve(mg, (g.rs, g.rd), BIBFS_SHIPPED_CAP, 1024, mutant=mutant)
        assert (answers(again) == answers(base)).all()
        return
    name, keep, bound, what = KILLS[mutant]
    for side in sides:  # on the graph and on its transpose
        rows, base, cap, q = pick(side, name, keep)
        assert len(rows)
        if bound is not None:
            base = side.solve(rows, cap, q, bound=bound)
        res = side.solve(rows, cap, q, bound=bound, mutant=mutant)
        if what == "answer":
            assert (answers(base) != answers(res)).any(), (mutant, name)
        else:
            assert (answers(base) == answers(res)).all() and [r.entries for r in base] != [r.entries for r in res], (mutant, name)


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    read = lambda f: open(os.path.join(CSRC, f)).read()
    meet, walk, internal = read("pgq_meet.hip"), read("pgq_walk.h"), read("pgq_internal.h")
    num = lambda text, pattern: eval(re.search(pattern, text).group(1), {})
    kernel = meet[meet.index("void k_bibfs("):meet.index("// ---- path emission")]
    chunks = walk[walk.index("meet_walk_chunks("):]
    floors = re.findall(r"const int qcap = std::max\((\d+), (?:opt|options\(\))\.bibfs_queue\);", meet)
    assert len(floors) == 2 and len(set(floors)) == 1  # the chain and meet_bidirectional
    got = dict(
        queue_floor=int(floors[0]),
        cap_floor=num(meet, r"capb = \(int64_t\)std::max\((\d+), options\(\)\.bibfs_cap\);"),
        block=num(meet, r"__launch_bounds__\((\d+)\) void k_bibfs\("),
        walk_stride=num(kernel, r"nf\[side\], wib, (\d+), xoff, xadj,"),
        walk_lanes=num(chunks, r"pb \+= (\d+) \* stride"),
        chunk=num(chunks, r"q \+= (\d+);"),
        depth=num(meet, r"#define PGQ_BIBFS_DEPTH (\d+)"),
        rows=num(internal, r"int bibfs_rows = ([0-9 <*]+);"),
        rows_max=num(internal, r"int bibfs_rows_max = ([0-9 <*]+);"),
        rows_edges=num(meet, r"std::min<int64_t>\(opt\.bibfs_rows_max, c->E / (\d+)\)"),
        far_rows_start=num(internal, r"meet_far_rows \{ (\d+) \}"),
    )
    assert got == BIBFS_LIMITS
    assert num(internal, r"int bibfs_cap = ([0-9 <*]+);") == BIBFS_SHIPPED_CAP
    assert (M.WAVES, M.LANES, M.CHUNK, M.DEPTH) == (got["walk_stride"], got["walk_lanes"], got["chunk"], got["depth"]) and M.PASS == got["block"]
    # the decisions the model restates, as the kernel writes them
    for text in ("if (BND && lvl[0] + lvl[1] >= bound)", "const int side = work[0] <= work[1] ? 0 : 1;", "if (work[side] > cap) break;",
                 "if (nn > (u32)qcap) break;", "if (fresh && slot < (u32)qcap) nxt[slot] = xs[k];", "if (tn > (u32)qcap) {",
                 "if (first && slot < (u32)qcap) tlist[slot]", "if (tid == 0) s_tn = ~0u;", "i += gridDim.x", "meet_walk_chunks<PGQ_BIBFS_DEPTH>("):
        assert text in kernel, text
    assert kernel.index("lvl[0] + lvl[1] >= bound") < kernel.index("work[0] <= work[1]") < kernel.index("work[side] > cap")
    assert kernel.index("if (s_found) {") < kernel.index("if (nn == 0) {") < kernel.index("if (nn > (u32)qcap) break;")
    for text in ("const int cnt = min(64, (list_n - pb + stride - 1) / stride);", "q = b & ~3;", "if (e > b) {", "const int p = pb + lane * stride;"):
        assert text in chunks, text
    assert "const u32 grid = (u32)std::min<int64_t>(n, device_cus());" in meet
    assert "std::max(opt.bibfs_rows, (int)std::min<int64_t>(opt.bibfs_rows_max, c->E / 4096))" in meet
