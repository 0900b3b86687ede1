"""Static LDS of the bit-map kernels, read from the built libpgq_hip.so, against the host rules that place their maps.

The host decides from V alone whether a kernel's per-vertex (or frontier) bit map goes to LDS.  The decision adds the map
to a fixed allowance for the kernel's own __shared__ arrays (k_src_ball, k_meet4*, k_bibfs) or to the static size the HIP
runtime reports (k_pull_lanes, k_pull_sparse).  This file reads those static sizes from the gfx950 code objects and checks
that every map the host puts in LDS fits beside them, and recomputes every entry of helpers.LDS_LIMITS, the V edges that
test_lds_limits_gpu.py runs on both sides.  A compiler or kernel change that moves an edge fails here, before a GPU run."""
import os
import re
import shutil
import subprocess

import pytest

from duckpgq_extension_amd import binding
from helpers import LDS_LIMITS

ARCH_TRIPLE = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

LDS_ALL = 160 * 1024        # LDS per CU (gfx950)
MEET4_BUDGET = 150 * 1024   # option meet4_lds_kb, capped at 150 (pgq_meet.hip, MapPlan: lds_budget, kMapLdsKB)
BALL_ROW_STATE = 23 * 1024  # what MapPlan keeps for k_src_ball's own arrays (kBallRowState)
WDS = (1, 2, 4, 8, 16, 32)


def tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    assert p, "%s not found (ROCm's LLVM tools read the code objects of libpgq_hip.so)" % name
    return p


def parse_kernel(mangled):
    """'_ZN3pgq12k_pull_lanesILi32ELi1ELb1EEEv...' -> ('k_pull_lanes', (32, 1, 1)); None for other symbols."""
    m = re.match(r"_ZN3pgq(\d+)", mangled)
    if not m:
        return None
    at = m.end()
    name = mangled[at:at + int(m.group(1))]
    rest = mangled[at + int(m.group(1)):]
    args = ()
    if rest.startswith("I"):
        targs = re.match(r"I((?:L[ib]\d+E)*)E", rest)
        if targs:
            args = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", targs.group(1)))
    return name, args


@pytest.fixture(scope="module")
def static_lds(tmp_path_factory):
    """{(kernel name, template args): .group_segment_fixed_size} over every gfx950 code object in the library."""
    lib = binding.lib_paths()[0]
    assert os.path.exists(lib), "libpgq_hip.so is not built: run build() first"
    tmp = tmp_path_factory.mktemp("fatbin")
    fatbin = tmp / "hip_fatbin"
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=%s" % fatbin, lib, str(tmp / "lib_copy")])
    data = fatbin.read_bytes()
    # one bundle per translation unit, each starting with the magic
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    sizes = {}
    for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle, co = tmp / ("tu%d.bundle" % k), tmp / ("tu%d.co" % k)
        bundle.write_bytes(data[a:b])
        subprocess.check_call([tool("clang-offload-bundler"), "--type=o", "--targets=" + ARCH_TRIPLE, "--input=%s" % bundle,
                               "--output=%s" % co, "--unbundle"])
        notes = subprocess.check_output([tool("llvm-readelf"), "--notes", str(co)], text=True)
        entry = {}
        for line in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(name|group_segment_fixed_size):\s+(\S+)", line)
            if not m:
                continue
            entry[m.group(1)] = m.group(2)
            if len(entry) == 2:  # both keys of one kernel's map seen, in whichever order
                key = parse_kernel(entry["name"])
                if key:
                    sizes[key] = int(entry["group_segment_fixed_size"])
                entry = {}
    return sizes


def one_size(static_lds, name, pick):
    """The static LDS of every instantiation of `name` whose template args satisfy `pick`; they must agree (the host's rule
    uses the one the options select, and the table has one edge per row)."""
    found = {args: v for (n, args), v in static_lds.items() if n == name and pick(args)}
    assert found, "no instantiation of %s in libpgq_hip.so" % name
    assert len(set(found.values())) == 1, "%s: static LDS differs between instantiations %s" % (name, found)
    return next(iter(found.values()))


def largest(fits):
    """The largest V in [1, 2^24) for which fits(V) holds; fits is monotone (true up to the edge)."""
    lo, hi = 1, 1 << 24
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def bm_bytes(V):
    return ((V + 127) // 128) * 4 * 4  # bm_words = ceil(V / 128) * 4 (pgq_meet.hip, MapPlan)


# ---- the host rules, as written in the library ---------------------------------------------------------------------------

def ball_lds(V):  # pgq_meet.hip, MapPlan: ball_lds
    return bm_bytes(V) + BALL_ROW_STATE <= min(LDS_ALL, MEET4_BUDGET + BALL_ROW_STATE)


def ball_two_per_cu(V):  # ... ball_two: two workgroups per CU when both fit (PGQ_BALL_WAVES = 8)
    return 2 * (bm_bytes(V) + BALL_ROW_STATE) <= LDS_ALL


def meet4_lds(V):  # ... lds_map
    return bm_bytes(V) + 2048 <= MEET4_BUDGET


def bibfs_lds(V):  # ... bi_lds: two maps of bm_words + 4 words
    return 2 * (bm_bytes(V) // 4 + 4) * 4 + 2048 <= MEET4_BUDGET


def pull_lanes_lds(V, static):  # pgq_lanes.hip, launch_lanes: lds_map (sl = static size + 1)
    n_blk = (V + 63) // 64
    dyn = n_blk * 8 + ((n_blk + 1) & ~1) * 2 + (n_blk // 8 + 2) * 4 + 16  # kGroupBlocks = 8
    return (static + 1) + dyn + 256 <= LDS_ALL


def pull_sparse_lds(V, static):  # pgq_msbfs.hip, pull_sparse / launch_pull_sparse: lds_map
    bit_words = ((V + 63) // 64) * 2 + 2
    return (static + 1) + bit_words * 6 + 256 <= LDS_ALL


def lcc_big_lds(V):  # pgq_analytics.hip, lcc_device: in_lds (bm_words = ceil(V / 32))
    return ((V + 31) // 32) * 4 + 256 <= 150 * 1024


# ---- budgets ------------------------------------------------------------------------------------------------------------

def test_src_ball_static_lds_leaves_room_for_its_map(static_lds):
    # the host keeps 23 KB for k_src_ball's own arrays and gives its map up to 137 KB of dynamic LDS (its attribute)
    for gm in (0, 1):  # k_src_ball<GM, TRACE>: the map in LDS / in global memory
        s = one_size(static_lds, "k_src_ball", lambda a, gm=gm: a[0] == gm)
        assert s <= BALL_ROW_STATE, "k_src_ball uses %d B of static LDS, over the %d B row_state of meet_prepass" % (s, BALL_ROW_STATE)
    assert bm_bytes(LDS_LIMITS["ball_1_per_cu"]) <= 137 * 1024  # the MaxDynamicSharedMemorySize meet_attributes() sets (kBallLdsAttr)


@pytest.mark.parametrize("name,pick,maps", [("k_meet4d", lambda a: a[0] == 0, 1), ("k_meet4", lambda a: a[1] == 0, 1),
                                            ("k_bibfs", lambda a: a[0] == 0, 2)])
def test_meet_kernels_static_lds_plus_largest_map_fit(static_lds, name, pick, maps):
    # the LDS variants (k_meet4d<false, *>, k_meet4<true, false>, k_bibfs<false>): the largest map the host puts in LDS fits
    # the 150 KB budget beside 2 KB of reserve; with the kernel's static arrays it must fit the CU, and it must not exceed
    # the 150 KB attribute meet_attributes() sets
    s = one_size(static_lds, name, pick)
    if maps == 2:
        largest_map = 2 * (bm_bytes(largest(bibfs_lds)) // 4 + 4) * 4
    else:
        largest_map = bm_bytes(largest(meet4_lds))
    assert largest_map <= MEET4_BUDGET
    assert s + largest_map <= LDS_ALL, "%s: %d B static + %d B map > %d B" % (name, s, largest_map, LDS_ALL)


# ---- the edges test_lds_limits_gpu.py runs ------------------------------------------------------------------------------

def msg(row):
    return "helpers.LDS_LIMITS[%r] no longer matches the host rule and the built kernels: update that entry" % (row,)


def test_meet_kernel_edges_match_the_host_rules():
    assert largest(ball_two_per_cu) == LDS_LIMITS["ball_2_per_cu"], msg("ball_2_per_cu")
    assert largest(ball_lds) == LDS_LIMITS["ball_1_per_cu"], msg("ball_1_per_cu")
    assert largest(meet4_lds) == LDS_LIMITS["meet4"], msg("meet4")
    assert largest(bibfs_lds) == LDS_LIMITS["bibfs"], msg("bibfs")


def test_lcc_big_edge_matches_the_host_rule(static_lds):
    # k_lcc_big keeps 256 B for its own __shared__ state beside the map and asks for up to 150 KB of dynamic LDS
    limit = largest(lcc_big_lds)
    assert limit == LDS_LIMITS["lcc_big"], msg("lcc_big")
    s = one_size(static_lds, "k_lcc_big", lambda a: True)
    assert s <= 256, "k_lcc_big uses %d B of static LDS, over the 256 B lcc_device keeps for it" % s
    assert s + ((limit + 31) // 32) * 4 <= LDS_ALL


@pytest.mark.parametrize("wd", WDS)
def test_lane_kernel_edges_match_the_static_lds(static_lds, wd):
    s = one_size(static_lds, "k_pull_lanes", lambda a: a[0] == wd and a[2] == 1)
    assert largest(lambda V: pull_lanes_lds(V, s)) == LDS_LIMITS["pull_lanes"][wd], \
        msg("pull_lanes") + " [%d] (k_pull_lanes<%d, *, true>: %d B static)" % (wd, wd, s)
    s = one_size(static_lds, "k_pull_sparse", lambda a: a[0] == wd and a[2] == 16)
    assert largest(lambda V: pull_sparse_lds(V, s)) == LDS_LIMITS["pull_sparse"][wd], \
        msg("pull_sparse") + " [%d] (k_pull_sparse<%d, *, 16, *>: %d B static)" % (wd, wd, s)
