"""CPU checks of the degree-ordered packed lists and their two-part walk (duckpgq-extension_amd/csrc/pgq_pack.h:
pack_order_bucket, pack_head_groups, pack_part), through a g++ shim built like test_packed_layout_cpu.py's.

The walk model below follows the rules k_meet3 applies around seg_walk (pgq_meet.hip, pgq_walk.h): rounds of 64 descriptors,
requests of 64 groups of ONE part of the round's lists, DEPTH requests per pass (a processed slot is refilled first), the
stop and the cap looked at after every pass, `resume` = the round of the earliest unprocessed request; heads of all rounds
first, then the tails under what is left of the cap; a walk cut among the heads hands the row on with resume = 0, one cut
among the tails with the tails' resume, and "distance >= 4" is only claimed when both parts ran to their ends.  The stage
behind (k_meet4d) walks whole lists from `resume` on.  The model must give the single-part walk's membership answer; two
deliberately wrong variants of the rules must not."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckpgq-extension_amd", "csrc")

SHIM = r"""
#include "pgq_pack.h"
using namespace pgq;
extern "C" {
int shim_bucket(unsigned len) { return pack_order_bucket(len); }
unsigned shim_head_groups(unsigned ng) { return pack_head_groups(ng); }
void shim_part(unsigned len, int K, int part, int split, unsigned *out) {
	const PackPart p = pack_part(len, K, part, split != 0);
	out[0] = p.first;
	out[1] = p.groups;
	out[2] = p.entries;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the layout shim")
    d = tmp_path_factory.mktemp("order")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)],
                   check=True)
    lib = C.CDLL(str(so))
    lib.shim_bucket.restype = C.c_int
    lib.shim_bucket.argtypes = [C.c_uint]
    lib.shim_head_groups.restype = C.c_uint
    lib.shim_head_groups.argtypes = [C.c_uint]
    lib.shim_part.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.uint32)]
    return lib


def part(shim, n, K, which, split=1):
    out = np.zeros(3, dtype=np.uint32)
    shim.shim_part(n, K, which, split, out)
    return tuple(int(x) for x in out)  # first group, groups, entries


# ---- partition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 6])
def test_head_and_tail_cover_every_group_once(shim, K):
    for n in (0, 1, K - 1, K, K + 1, 4 * K - 1, 4 * K, 4 * K + 1, 8 * K + 1):
        ng = -(-n // K)
        hf, hg, he = part(shim, n, K, 0)
        tf, tg, te = part(shim, n, K, 1)
        assert hg == shim.shim_head_groups(ng) == (ng + 3) // 4
        groups = list(range(hf, hf + hg)) + list(range(tf, tf + tg))
        assert groups == list(range(ng)), (n, groups)  # heads first, every group exactly once
        assert he == min(n, hg * K) and he + te == n  # the entries of the two parts are the list's
        assert (hg > 0) == (n > 0)  # a list that has entries has a head; lists of up to K entries have no tail
        if n <= K:
            assert tg == 0 and te == 0
        assert part(shim, n, K, 0, split=0) == (0, ng, n)  # not split: part 0 is the whole list


def test_head_groups_exact_quarters(shim):
    assert [shim.shim_head_groups(g) for g in (0, 1, 2, 3, 4, 5, 8, 9)] == [0, 1, 1, 1, 1, 2, 2, 3]


# ---- bucket --------------------------------------------------------------------------------------------------------------
def test_bucket_is_floor_log2_and_monotone(shim):
    assert shim.shim_bucket(0) == 0 and shim.shim_bucket(1) == 0
    for k in range(1, 32):
        assert shim.shim_bucket(1 << k) == k
        assert shim.shim_bucket((1 << k) - 1) == max(k - 1, 0)
    assert shim.shim_bucket(0xFFFFFFFF) == 31
    lens = list(range(0, 5000)) + [int(x) for x in np.random.default_rng(1).integers(0, 1 << 32, 2000)]
    lens.sort()
    b = [shim.shim_bucket(x) for x in lens]
    assert all(x <= y for x, y in zip(b, b[1:]))
    assert all(0 <= x <= 31 for x in b)


# ---- walk model ------------------------------------------------------------------------------------------------------------
FAR = "distance >= 4"


def group_ids(lst, K, g):
    return [lst[min(g * K + k, len(lst) - 1)] for k in range(K)]  # padding repeats the last entry


def walk_part(shim, lists, K, which, split, member, cap, depth):
    """One seg_walk call over one part.  Returns (found, capped, resume, entries requested)."""
    reqs = []  # (first descriptor of the round, [(list, group)])
    for r0 in range(0, len(lists), 64):
        groups = []
        for j in range(r0, min(r0 + 64, len(lists))):
            first, ng, _ = part(shim, len(lists[j]), K, which, split)
            groups += [(j, first + g) for g in range(ng)]
        reqs += [(r0, groups[c:c + 64]) for c in range(0, len(groups), 64)]
    issued = min(depth, len(reqs))
    requested = K * sum(len(g) for _, g in reqs[:issued])
    done = 0
    while done < len(reqs):
        hi = min(done + depth, len(reqs))
        found = False
        for q in range(done, hi):
            if issued < len(reqs):  # the slot is refilled before its request is processed
                requested += K * len(reqs[issued][1])
                issued += 1
            found |= any(x in member for j, g in reqs[q][1] for x in group_ids(lists[j], K, g))
        done = hi
        resume = reqs[done][0] if done < len(reqs) else -(-len(lists) // 64) * 64
        if found:
            return True, False, resume, requested
        if requested > cap:
            return False, True, resume, requested
    return False, False, 0, requested


def next_stage(lists, member, resume):
    return 3 if any(x in member for lst in lists[resume:] for x in lst) else FAR


def row(shim, lists, K, member, cap, depth=2, variant=None):
    found, capped, resume, used = walk_part(shim, lists, K, 0, 1, member, cap, depth)
    if found:
        return 3
    if capped:  # cut among the heads: the tails of the rounds before are unwalked
        return next_stage(lists, member, resume if variant == "resume_is_cut_round" else 0)
    if variant == "known4_after_heads":
        return FAR
    found, capped, resume, _ = walk_part(shim, lists, K, 1, 1, member, cap - min(cap, used), depth)
    if found:
        return 3
    return next_stage(lists, member, resume) if capped else FAR


def single_part(shim, lists, K, member, cap, depth=2):
    found, capped, resume, _ = walk_part(shim, lists, K, 0, 0, member, cap, depth)
    if found:
        return 3
    return next_stage(lists, member, resume) if capped else FAR


@pytest.mark.parametrize("K", [5, 6])
def test_two_part_walk_gives_the_single_part_answer(shim, K):
    rng = np.random.default_rng(40 + K)
    seen = set()
    for trial in range(120):
        n = int(rng.choice([1, 3, 63, 64, 65, 130]))
        lens = rng.choice([0, 1, K - 1, K, K + 1, 4 * K, 4 * K + 1, 5 * K, 37], n)
        lists = [rng.integers(0, 4000, int(m)).tolist() for m in lens]
        flat = [x for lst in lists for x in lst]
        member = set()
        if flat and trial % 3:
            member = {flat[int(rng.integers(0, len(flat)))]}  # one witness somewhere (its duplicates are witnesses too)
        truth = 3 if any(x in member for x in flat) else FAR
        for cap in (1 << 30, int(rng.integers(1, 3000)), 0):
            for depth in (2, 4):
                got = row(shim, lists, K, member, cap, depth)
                assert got == truth, (trial, n, cap, depth)
                assert single_part(shim, lists, K, member, cap, depth) == truth
                seen.add((truth, cap < 1 << 30))
    assert len(seen) == 4  # with and without a witness, cut and not cut


def tail_witness_rows(K):
    """Two rounds of 64 lists of 8 groups each (head 2 groups, tail 6); the only member is the LAST entry of the first list: in
    round 0's tail."""
    lists = [list(range(1000 + 100 * j, 1000 + 100 * j + 8 * K)) for j in range(128)]
    return lists, {lists[0][-1]}


@pytest.mark.parametrize("K", [5, 6])
def test_wrong_variant_resume_is_the_cut_round(shim, K):
    lists, member = tail_witness_rows(K)
    # heads: two requests per round.  The first pass processes round 0's heads with round 1's already requested: 4 x 64 x K
    # entries requested > cap, the walk is cut with its earliest unprocessed request in round 1 (descriptor 64)
    cap = 3 * 64 * K
    found, capped, resume, _ = walk_part(shim, lists, K, 0, 1, member, cap, 2)
    assert (found, capped, resume) == (False, True, 64)
    assert row(shim, lists, K, member, cap) == 3
    assert row(shim, lists, K, member, cap, variant="resume_is_cut_round") == FAR  # round 0's tails were never walked


@pytest.mark.parametrize("K", [5, 6])
def test_wrong_variant_known4_after_the_heads(shim, K):
    lists, member = tail_witness_rows(K)
    assert row(shim, lists, K, member, 1 << 30) == 3
    assert row(shim, lists, K, member, 1 << 30, variant="known4_after_heads") == FAR


@pytest.mark.parametrize("K", [5, 6])
def test_cut_among_the_tails_resumes_in_the_tails_round(shim, K):
    lists, _ = tail_witness_rows(K)
    member = {lists[127][-1]}  # in round 1's tail
    heads = 4 * 64 * K  # every head request
    cap = heads + 64 * K  # the tails are cut after their first pass
    found, capped, resume, used = walk_part(shim, lists, K, 0, 1, member, cap, 2)
    assert (found, capped, used) == (False, False, heads)
    found, capped, resume, _ = walk_part(shim, lists, K, 1, 1, member, cap - used, 2)
    assert (found, capped, resume) == (False, True, 0)  # round 0's tails are 6 requests: still in round 0
    assert row(shim, lists, K, member, cap) == 3


def test_short_lists_have_empty_tails_and_pass_through(shim):
    K = 6
    lists = [[7 + j] * (1 + j % K) for j in range(130)]  # 1 .. K entries: no tail anywhere
    assert all(part(shim, len(lst), K, 1)[1] == 0 for lst in lists)
    assert row(shim, lists, K, {7 + 129}, 1 << 30) == 3
    assert row(shim, lists, K, {5}, 1 << 30) == FAR
