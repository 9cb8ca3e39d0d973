"""A pure-Python mirror of the host schedule of the leave-one-out pass: build_loo_tasks and the grid size of launch_loo in
patchmixturekriging_amd/csrc/pmk_loo.hip, plus the column geometry of loo_strip_kernel that a patch size decides (tile
count, strips, the 32-row pairs of the last block row).  No device and no library needed: the tests use it to PROVE that a
list of patch sizes drives a given branch before they look at any number (tests/test_loo_schedule_model.py on the CPU
with num_cu = 256, tests/test_gpu_loo_schedule.py with the device's count).

The comments name the host code each part mirrors; build_loo_tasks points back here.  If the schedule changes, change
both.
"""
from collections import namedtuple

TILE = 128
NQ = 8                                                  # one queue per XCD

Task = namedtuple("Task", "patch strip queue cost")


def tiles(n):
    return (n + TILE - 1) // TILE                       # pmk_model_create_ex: d.nt


def last_pairs(n):
    """loo_strip_kernel: rows of the last block row that are not identity padding, in 32-row pairs"""
    return (n - (tiles(n) - 1) * TILE + 31) >> 5


def tasks(sizes):
    """build_loo_tasks -> (tasks in device order, queue offsets [9]): queue x holds tasks [off[x], off[x + 1])"""
    nts = [tiles(n) for n in sizes]
    P = len(nts)
    load = [0] * NQ
    lightest = lambda: load.index(min(load))            # std::min_element: the first of equal minima
    # whole patches go to the lightest queue, largest first (std::stable_sort by nt); with fewer patches than queues
    # single tasks do
    order = sorted(range(P), key=lambda r: -nts[r])
    dealt = []
    for r in order:
        nt = nts[r]
        x = lightest()
        st = 0
        while 2 * st < nt:
            ln = nt - 2 * st
            if P < NQ:
                x = lightest()
            dealt.append(Task(r, st, x, ln * ln))
            load[x] += ln * ln
            st += 1
    # grouped by queue, longest first inside a queue (std::stable_sort)
    out = sorted(dealt, key=lambda t: (t.queue, -t.cost))
    off = [0] * (NQ + 1)
    for t in out:
        off[t.queue + 1] += 1
    for x in range(NQ):
        off[x + 1] += off[x]
    return out, off


def slots(sizes, num_cu):
    """launch_loo: the grid, min(tasks, num_cu) workgroups, each with one strip workspace"""
    return min(len(tasks(sizes)[0]), num_cu)


BRANCHES = ["p_lt_8", "p_ge_8", "tasks_gt_slots", "tasks_lt_8", "queue_longer_than_its_workgroups", "odd_nt", "even_nt",
            "last_pairs_1", "last_pairs_2", "last_pairs_3", "last_pairs_4", "half1_first_is_last", "nt_1"]


def branches(sizes, num_cu):
    """the names (out of BRANCHES) of what a leave-one-out pass over patches of these sizes drives"""
    hit = set()
    ts, off = tasks(sizes)
    grid = slots(sizes, num_cu)
    hit.add("p_lt_8" if len(sizes) < NQ else "p_ge_8")
    if len(ts) > grid:
        hit.add("tasks_gt_slots")                       # pigeonhole: some workgroup reuses its strip workspace
    if len(ts) < NQ:
        hit.add("tasks_lt_8")                           # fewer workgroups than queues
    for x in range(NQ):
        own = len(range(x, grid, NQ))                   # workgroups with blockIdx.x & 7 == x
        if off[x + 1] - off[x] > own:
            hit.add("queue_longer_than_its_workgroups")     # the others must take what is left
    for n in sizes:
        nt = tiles(n)
        hit.add("odd_nt" if nt & 1 else "even_nt")      # odd: the last strip has 128 columns and four idle waves
        hit.add("last_pairs_%d" % last_pairs(n))
        if nt % 2 == 0:
            # the last strip is s = nt / 2 - 1, i0 = nt - 2; its second half starts at w0 = nt - 1, the last block row,
            # with nb = 0: identity slice, padded-row skip and empty GEMM in one call
            hit.add("half1_first_is_last")
        if nt == 1:
            hit.add("nt_1")
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_loo_schedule.py.  They live here so that the CPU test can prove what they cover.
# ---------------------------------------------------------------------------------------------------------------------
REMAINDERS = [1, 32, 33, 64, 65, 96, 97, 128]           # both sides of every 32-row pair edge of the last block row


def pool_sizes():
    """part A: n = 128 (nt - 1) + r for nt = 1..5 and every remainder, 40 sizes up to 640 (n = 1 among them), in a fixed
    interleaving (stride 17), so that the prefixes of 7, 8 and 9 are ragged"""
    pool = [TILE * (nt - 1) + r for nt in range(1, 6) for r in REMAINDERS]
    n = len(pool)
    return [pool[(17 * i + 5) % n] for i in range(n)]


def deep_sizes():
    """part A: 12 tiles with 97 rows in the last, 13 tiles with one: strips that start at block rows 2 to 12"""
    return [TILE * 11 + 97, TILE * 12 + 1]


def repeats_beyond(sizes, num_cu):
    """how often `sizes` is repeated so that the tasks are more than 1.5 times the workgroups of a full grid"""
    per = len(tasks(sizes)[0])
    return (3 * num_cu) // (2 * per) + 1


def compositions(npool, seed=2025):
    """name -> pool indices scored together: the pool, reversed, one fixed permutation, prefixes on both sides of the
    P < 8 rule"""
    import numpy as np
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(npool).tolist()
    comps = {"pool": list(range(npool)), "reversed": list(range(npool))[::-1], "permuted": perm}
    for P in (7, 8, 9):
        comps["prefix%d" % P] = list(range(P))
    return comps


def exact_batches(num_cu):
    """part A: name -> patch sizes.  (The batch of interleaved patterns, 'repeated', is this pool repeats_beyond() times
    over.)"""
    pool, deep = pool_sizes(), deep_sizes()
    out = {name: [pool[i] for i in idx] for name, idx in compositions(len(pool)).items()}
    out["deep12_alone"] = [deep[0]]
    out["deep13_alone"] = [deep[1]]
    out["deep12_and_seven_small"] = [deep[0]] + [pool[i] for i in range(len(pool)) if tiles(pool[i]) == 1][:7]
    out["repeated"] = pool * repeats_beyond(pool, num_cu)
    return out


def fitted_pool_sizes():
    """part B: 24 of the sizes of part A, ragged, every tile count 1..5 and every remainder (n = 1 among them)"""
    pool = pool_sizes()
    picked = [pool[i] for i in range(0, len(pool), 2)] + [1, 128, 257, 640]
    assert len(picked) == 24
    return picked


def fitted_batches(num_cu):
    """part B: name -> indices into fitted_pool_sizes()"""
    sizes = fitted_pool_sizes()
    comps = compositions(len(sizes), seed=2026)
    out = {k: comps[k] for k in ("pool", "reversed", "permuted", "prefix7", "prefix9")}
    out["repeated"] = list(range(len(sizes))) * repeats_beyond(sizes, num_cu)
    return out


EVIDENCE_SIZES = [1, 15, 16, 17, 255, 256, 257, 300]    # part C: the 16-row stride of the R-column kernels, and 256 threads


def coverage(num_cu):
    """{branch: [batches of part A that drive it]}"""
    cov = {}
    for name, sizes in exact_batches(num_cu).items():
        for b in branches(sizes, num_cu):
            cov.setdefault(b, []).append(name)
    return cov
