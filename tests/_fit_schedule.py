"""A pure-Python mirror of the host schedule of the fit path: launch_cholesky and launch_split_solves in
patchmixturekriging_amd/csrc/pmk_chol.hip, plus the two mode rules of pmk_api.cpp (pmk_model_create_ex chooses the
split path by size, pmk_test_model_set_split forces it).  No device and no library needed: the tests use it to PROVE that
a list of patch sizes drives a given branch of the schedule before they look at any number
(tests/test_fit_schedule_model.py on the CPU with num_cu = 256, tests/test_gpu_fit_schedule.py with the device's count).

The comments name the host code each part mirrors; launch_cholesky points back here.  If the schedule changes, change
both.
"""
from collections import namedtuple

TILE = 128

# one iteration of launch_cholesky's loop over l.  `pending` is what the partial launch of a split step is handed by the
# split step before it, (n, G, nsplit), or None: the first `n` workgroups of chol_partial_kernel factorise the diagonal
# tiles that step left behind (pot_nsplit = 0 where the step launch folded their partial sums into the slab already).
# `flush_before` is the mid-loop flush_pending(): a potrf-only launch in front of a batched step that follows a split one.
Launch = namedtuple("Launch", "l nactive G nsplit fold pending flush_before partial_grid step_grid half")
Schedule = namedtuple("Schedule", "sizes nts max_nt order split launches final_flush half_tiles solves chain_blocks")


def tiles(n):
    return (n + TILE - 1) // TILE                       # pmk_model_create_ex: d.nt


def auto_split(nts, num_cu):
    """pmk_model_create_ex: m->split_mode = max_nt >= 32 && P * (max_nt - 1) / 2 < 2 * num_cu"""
    max_nt = max(nts)
    return max_nt >= 32 and len(nts) * (max_nt - 1) // 2 < 2 * num_cu


def nsplit_of(l, G, num_cu, split):
    """launch_cholesky: nsplit_of(l, G) with want_wg = 2 * num_cu"""
    want_wg = 2 * num_cu
    if not (split and l >= 4):
        return 1
    return max(1, min(min(16, l // 2), (want_wg + G) // (G + 1)))


def schedule(sizes, num_cu, mode=None):
    """sizes: points per patch in the caller's order.  mode: None = what the library decides by itself, 0..3 = what
    pmk_test_model_set_split(m, mode) forces (0 batched; 1 split, solves by size; 2 split, block-by-block solves;
    3 split, chained solves)."""
    nts = [tiles(n) for n in sizes]
    P, max_nt = len(nts), max(nts)
    # pmk_model_create_ex: std::stable_sort by nt, largest first; active_prefix[t] = patches with nt >= t
    order = sorted(range(P), key=lambda r: -nts[r])
    active_prefix = [sum(1 for nt in nts if nt >= t) for t in range(max_nt + 2)]
    if mode is None:
        split, chain_mode = auto_split(nts, num_cu), -1
    else:
        split = mode != 0 and max_nt >= 2               # pmk_test_model_set_split
        chain_mode = {2: 0, 3: 1}.get(mode, -1)
    ns = lambda l, G: nsplit_of(l, G, num_cu, split)
    # the sizing pass: both halves of the partial buffer hold the largest step
    half_tiles = 0
    for l in range(max_nt - 1):
        na, G = active_prefix[max_nt - l], max_nt - l - 1
        if ns(l, G) > 1:
            half_tiles = max(half_tiles, na * (G + 1) * ns(l, G))
    launches, pend = [], None                           # pend = (n, G, nsplit) <-> struct Pending
    for l in range(max_nt - 1):
        nactive = active_prefix[max_nt - l]             # patch p runs k = l - (max_nt - nt_p): active when nt_p >= max_nt - l
        G = max_nt - l - 1
        if nactive == 0:
            continue
        nsplit = ns(l, G)
        grid = 8 * ((nactive + 7) // 8) * G             # padded for step_slot's deal over 8 XCDs
        if nsplit > 1:
            fold = G >= 2 and (l + 1) <= 4 * ns(l + 1, G - 1)
            npot = pend[0] if pend else 0
            launches.append(Launch(l, nactive, G, nsplit, fold, pend, False, npot + nactive * (G + 1) * nsplit,
                                   grid + (nactive if fold else 0), l & 1))
            pend = (nactive, G, 0 if fold else nsplit)
        else:
            launches.append(Launch(l, nactive, G, 1, False, None, pend is not None, 0, grid, None))
            pend = None                                 # flush_pending() ran (a no-op when nothing was pending)
    final_flush = pend                                  # the flush_pending() after the loop: a potrf-only launch
    # launch_backsolve / launch_split_solves
    if not split:
        solves, chain_blocks = "backsolve", 0
    else:
        chain = (chain_mode != 0) if chain_mode >= 0 else P * max_nt <= 2 * num_cu
        solves, chain_blocks = ("chained" if chain else "blocks"), P * max_nt
    return Schedule(list(sizes), nts, max_nt, order, split, launches, final_flush, half_tiles, solves, chain_blocks)


def step_slots(nactive, G):
    """step_slot of the batched step kernel, for every block of the padded grid: {block id: (slot, bx)}, surplus blocks
    left out.  A correct deal reaches every (slot, bx) with slot < nactive, bx < G exactly once."""
    out = {}
    for b in range(8 * ((nactive + 7) // 8) * G):
        xcd, idx = b & 7, b >> 3
        per = (nactive - xcd + 7) >> 3
        if idx >= per * G:
            continue
        if idx < per:
            loc, bx = idx, 0
        else:
            j = idx - per
            loc, bx = j // (G - 1), 1 + j % (G - 1)
        out[b] = (xcd + 8 * loc, bx)
    return out


def branches(sched, auto_solves=False):
    """the names of the schedule branches a fit with this schedule drives (the coverage list of the edge cases)"""
    hit = set()
    ls = sched.launches
    by_l = {L.l: L for L in ls}
    if sched.split:
        if 3 in by_l and 4 in by_l and by_l[3].nsplit == 1 and by_l[4].nsplit > 1:
            hit.add("nsplit 1 -> >1 at l = 4")
        if any(L.nsplit > 1 and L.G == 1 for L in ls):
            hit.add("split step with G = 1")
        if any(L.nsplit > 1 and L.fold for L in ls) and any(L.nsplit > 1 and not L.fold for L in ls):
            # every fit of seven tiles or more has this: its last launch has G = 1, where there is nothing to fold
            hit.add("fold on, and off at G = 1, in one fit")
        # the switch proper, (l + 1) <= 4 * nsplit_of(l + 1, G - 1), turning fold off: reported, not required (at 256
        # CUs it needs more than 64 tiles, see tests/test_fit_schedule_model.py)
        if any(L.nsplit > 1 and L.G >= 2 and not L.fold for L in ls):
            hit.add("fold off with G >= 2")
        if any(L.pending and L.pending[0] < L.nactive for L in ls):
            hit.add("pending launch with pend.n < nactive")
        if any(L.pending and L.pending[2] == 0 for L in ls):
            hit.add("pending tile folded already (pot_nsplit = 0)")
        if sched.final_flush:
            hit.add("final potrf-only flush")
        if any(nt == 1 for nt in sched.nts):
            hit.add("nt = 1 patch in a split batch")
        if any(L.flush_before for L in ls):
            hit.add("mid-loop flush")
        # nsplit_of's third term: fewer chunks than min(16, l / 2) because one patch's tiles fill the chip already
        if any(L.nsplit > 1 and L.nsplit < min(16, L.l // 2) for L in ls):
            hit.add("chip-filling bound on nsplit binds")
        if auto_solves:
            hit.add("solves by size: " + sched.solves)
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_fit_schedule.py.  They live here so that the CPU test can prove what they cover.
# ---------------------------------------------------------------------------------------------------------------------
def pool_sizes():
    """part A: about 40 patch sizes, in the caller's order (interleaved: a patch's slot in a launch is not its index, and
    the prefixes of 7..17 patches are ragged too).  One-tile sizes 1, 31, 32, 33, 127, 128; both sides of every tile edge
    up to 12 tiles; two patches of more than 20 tiles; duplicates."""
    one = [1, 31, 32, 33, 127, 128]
    edges = []
    for e in range(1, 12):
        edges += [128 * e + 1, 128 * (e + 1)]           # first and last size of e + 1 tiles
    edges += [128 * 3 - 1, 128 * 6 - 1, 128 * 9 - 1]    # one short of an edge
    big = [2561, 2700]                                  # 21 and 22 tiles
    dup = [640, 640, 300, 300, 1000, 1000, 700]         # with these the active count visits every residue mod 8
    pool = one + edges + big + dup
    # a fixed interleaving: stride through the list (40 patches, stride 17)
    n = len(pool)
    return [pool[(17 * i + 5) % n] for i in range(n)]


def pool_compositions(npool, seed=2024):
    """part A: name -> list of pool indices fitted together (the 'alone' and 'beside the largest' compositions are one
    model per patch and are built by the test)"""
    import numpy as np
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(npool).tolist()
    comps = {"pool": list(range(npool)), "reversed": list(range(npool))[::-1], "permuted": perm}
    for P in (7, 8, 9, 15, 16, 17):
        comps["prefix%d" % P] = list(range(P))
    return comps


def _off(nt, which):
    """a size of nt tiles: the full tile count, one point short, or one row in the last tile"""
    return {"full": TILE * nt, "short": TILE * nt - 1, "row": TILE * (nt - 1) + 1}[which]


def edge_cases():
    """part C: name -> patch sizes (points).  Tile counts in the names; sizes are deliberate off-multiples of 128."""
    cases = {}
    for nt in (2, 3, 5, 6, 7, 9):
        for which in ("full", "short", "row"):
            cases["single_%dt_%s" % (nt, which)] = [_off(nt, which)]
    # tiles 40, 2, 1, 39, 17, 1, 6: the one-tile patches never enter the loop, the two-tile one enters at the last launch
    cases["ragged_40_2_1_39_17_1_6"] = [5120, 200, 77, 4865, 2049, 128, 767]
    cases["ragged_33_32_32_9_5"] = [4097, 4096, 3969, 1100, 513]
    # max_nt = 12: splitting starts at l = 4 with one patch; the 7-tile patch enters at l = 5, the 6-tile one at l = 6
    cases["enter_after_split_12_7_6"] = [1536, 800, 641]
    # many large patches, ragged by one tile and by residues: 7 x 24..26 tiles (block-by-block solves by size at 256 CUs:
    # 7 * 26 = 182 blocks fit, so this one is chained; the nine 33-tile patches of test_gpu_parity.py are not)
    cases["seven_large_26_25_24"] = [3328, 3201, 3200, 3073, 3072, 2945, 3327]
    # more blocks than 2 * num_cu, so that the solves go block by block by size: 90 patches of 5..7 tiles (630 block slots
    # at 256 CUs) -- and split steps with up to 90 patch slots
    cases["many_small_90x5_6_7"] = [896 - 128 * (r % 3) - (r % 7) for r in range(90)]
    return cases


REQUIRED_BRANCHES = [
    "nsplit 1 -> >1 at l = 4",
    "split step with G = 1",
    "fold on, and off at G = 1, in one fit",
    "pending launch with pend.n < nactive",
    "final potrf-only flush",
    "solves by size: chained",
    "solves by size: blocks",
    "nt = 1 patch in a split batch",
]


def coverage(num_cu):
    """{branch: [cases that drive it]} over edge_cases() in forced mode 1 (split, solves chosen by size)"""
    cov = {}
    for name, sizes in edge_cases().items():
        for b in branches(schedule(sizes, num_cu, 1), auto_solves=True):
            cov.setdefault(b, []).append(name)
    return cov
