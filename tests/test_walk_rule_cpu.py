"""The stop rule of the walk calls (csrc/pgq_walk_rule.h: WalkQuery, WalkRule, WalkRow, WalkPlan) without a GPU: walk_rule_main.cpp,
compiled by g++ against that header alone, is fed every sequence W_lo .. W_K[dst] of at most 5 lengths over {0, 1, P-1, P, P+1,
INT64_MAX} for P = k in {1, 2, 16}, g in {1, 2, 3} and SHORTEST k, lo in {0, 1, 2}, by rounds and by distance, and what it prints
— the row behind every round, the plan, the plan fed one walk at a time — is held against the Python models:
    k_groups_model._open_after and _cut          the groups, by rounds and by distance
    path_modes_model.rounds_needed               SHORTEST k by distance
    the `ck` loop of k_walks_model.solve         SHORTEST k by rounds (transcribed below: the loop sits inside solve)"""
import itertools
import os
import subprocess

import pytest

import k_groups_model as G
import k_walks_model as W
import path_modes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckpgq-extension_amd", "csrc")
INT64_MAX = W.INT64_MAX


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("walk_rule") / "walk_rule"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "walk_rule_main.cpp")])
    return str(exe)


def ck_loop(per_len, k):
    """k_walks_model.solve's loop over a row's lengths without the unranking: (ck, walks taken, their elements, lengths taken from,
    lengths added)."""
    walks = ck = el = emitted = fed = 0
    for t, w in per_len:
        if walks >= k or ck >= k:
            break
        if w > 0:
            ck = W._add(ck, w, None)
            take = min(w, k - walks)
            walks, el, emitted, fed = walks + take, el + take * (2 * t + 1), emitted + 1, fed + 1
    return ck, walks, el, emitted, fed


def cases(P, lo):
    """(lo, g, limit, by_distance, [W_0 .. W_K]): g = 0 is SHORTEST k.  Below lo the row has no walk — and, by distance, also one
    at t = 0: a distance below lo, a row that never closes."""
    values = sorted({0, 1, P - 1, P, P + 1, INT64_MAX})
    for n in range(1, 6):
        for seq in itertools.product(values, repeat=n):
            for g in (0, 1, 2, 3):
                yield lo, g, P, 0, [0] * lo + list(seq)
                yield lo, g, P, 1, [0] * lo + list(seq)
                if lo > 0:
                    yield lo, g, P, 1, [1] + [0] * (lo - 1) + list(seq)


@pytest.mark.parametrize("lo", (0, 1, 2))
@pytest.mark.parametrize("P", (1, 2, 16))
def test_rule_against_the_models(rule_exe, P, lo):
    todo = list(cases(P, lo))
    text = "".join("%d %d %d %d %d %s\n" % (lo, g, limit, bd, len(ws), " ".join(map(str, ws))) for lo, g, limit, bd, ws in todo)
    out = subprocess.run([rule_exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(todo)
    closed_early = cut_inside = saturated = 0
    for (_, g, limit, bd, ws), line in zip(todo, out):
        what = (lo, g, limit, bd, ws)
        got = [int(x) for x in line.split()]
        K = len(ws) - 1
        assert len(got) == 3 * (K - lo + 1) + 8, what
        Ws = [{0: w} if w else {} for w in ws]
        per_len = [(t, ws[t]) for t in range(lo, K + 1)]
        rounds, plan, plan1 = got[:-8], tuple(got[-8:-4]), tuple(got[-4:])
        for t in range(lo, K + 1):
            count, groups, is_open = rounds[3 * (t - lo):3 * (t - lo) + 3]
            upto = per_len[:t - lo + 1]
            if g == 0 and not bd:
                ck, _, _, _, fed = ck_loop(upto, limit)
                assert (count, groups, is_open) == (ck, fed, int(ck < limit)), (what, t)
            elif g == 0:
                closes = M.rounds_needed(Ws, 0, lo, K, limit)
                if t < K:
                    assert is_open == int(t < closes), (what, t)
                assert count == (0 if is_open else limit), (what, t)
            else:
                assert is_open == int(G._open_after(Ws, 0, lo, t, g, limit, G.SIMPLE if bd else G.WALK, None)), (what, t)
                if bd:
                    assert count == (0 if is_open else limit + 1), (what, t)
                else:
                    _, total, _ = G._cut(upto, g, limit, None)
                    assert min(count, limit + 1) == min(total, limit + 1) and groups <= g, (what, t)
                    if is_open:
                        assert (count, groups) == (total, sum(1 for _, w in upto if w > 0)), (what, t)
            closed_early += int(not is_open and t < K)
        if g == 0:
            ck, walks, el, emitted, _ = ck_loop(per_len, limit)
            want = (walks, el, emitted)
            # what the rounds left (by rounds: the walks of lo..T edges); what the search found
            counts = (rounds[-3] if bd else ck, min(sum(w for _, w in per_len), limit))
        else:
            kept, total, ngroups = G._cut(per_len, g, limit, None)
            want = (sum(n for _, n in kept), sum(n * (2 * t + 1) for t, n in kept), ngroups)
            counts = (min(total, limit + 1),) * 2
            cut_inside += int(any(n < dict(per_len)[t] for t, n in kept))
        assert (plan[0], plan[1], plan[3]) == want and plan[2] == counts[0], (what, plan, want, counts)
        assert (plan1[0], plan1[1], plan1[3]) == want and plan1[2] == counts[1], (what, plan1, want, counts)
        saturated += int(INT64_MAX in ws)
    assert closed_early and saturated and (cut_inside or P == 1)
