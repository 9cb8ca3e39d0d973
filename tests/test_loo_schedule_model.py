"""CPU tests of tests/_loo_schedule.py, the Python mirror of build_loo_tasks / launch_loo (csrc/pmk_loo.hip): that the
mirror deals every strip of every patch exactly once, and that the inputs of tests/test_gpu_loo_schedule.py drive the
branches they are meant to drive (at num_cu = 256, an MI355X; the dealing rules at 8, 64 and 304 as well)."""
import numpy as np

import _loo_schedule as S

NUM_CU = 256


def _sizes_of(nts):
    return [S.TILE * nt for nt in nts]


def _all_inputs(num_cu):
    rng = np.random.Generator(np.random.PCG64(31))
    inputs = dict(S.exact_batches(num_cu))
    fitted = S.fitted_pool_sizes()
    for name, idx in S.fitted_batches(num_cu).items():
        inputs["fitted_" + name] = [fitted[i] for i in idx]
    inputs["evidence"] = list(S.EVIDENCE_SIZES)
    for k in range(20):                                 # and random ragged batches on both sides of 8 patches
        inputs["random%d" % k] = rng.integers(1, 2000, size=int(rng.integers(1, 30))).tolist()
    return inputs


def test_every_strip_is_dealt_exactly_once():
    for num_cu in (NUM_CU, 8, 64, 304):
        for name, sizes in _all_inputs(num_cu).items():
            ts, off = S.tasks(sizes)
            want = sorted((r, st) for r, n in enumerate(sizes) for st in range(S.tiles(n)) if 2 * st < S.tiles(n))
            assert sorted((t.patch, t.strip) for t in ts) == want, (num_cu, name)
            assert off[0] == 0 and off[-1] == len(ts) and off == sorted(off), (num_cu, name, off)
            for x in range(S.NQ):
                mine = ts[off[x]:off[x + 1]]
                assert all(t.queue == x for t in mine), (num_cu, name, x)
                costs = [t.cost for t in mine]
                assert costs == sorted(costs, reverse=True), (num_cu, name, x)        # longest first
            for t in ts:
                assert t.cost == (S.tiles(sizes[t.patch]) - 2 * t.strip) ** 2
            if len(sizes) >= 8:                         # all strips of a patch share a queue: one L2 streams one factor
                queue = {}
                for t in ts:
                    assert queue.setdefault(t.patch, t.queue) == t.queue, (num_cu, name, t)
            assert S.slots(sizes, num_cu) == min(len(ts), num_cu)


def test_figures_of_the_dealing_rule():
    ts, off = S.tasks(_sizes_of([12] + [1] * 7))
    assert len(ts) == 13 and off[1] - off[0] == 6 and all(t.patch == 0 for t in ts[:6])
    assert [t.strip for t in ts[:6]] == [0, 1, 2, 3, 4, 5]
    ts, off = S.tasks(_sizes_of([5] * 60 + [3] * 60 + [2] * 60 + [1] * 120))
    assert len(ts) == 480
    loads = [sum(t.cost for t in ts[off[x]:off[x + 1]]) for x in range(8)]
    assert min(loads) == 382 and max(loads) == 383, loads
    ts, off = S.tasks(_sizes_of([33]))
    assert len(ts) == 17 and all(off[x + 1] > off[x] for x in range(8))
    assert len(S.tasks(_sizes_of([3]))[0]) == 2
    # P < 8 deals task by task: the strips of the one patch are spread; P >= 8 keeps them together
    assert len({t.queue for t in S.tasks(_sizes_of([12] * 7))[0]}) == 8
    assert len({t.queue for t in S.tasks(_sizes_of([12] * 8))[0] if t.patch == 0}) == 1


def test_geometry_of_the_pool():
    pool = S.pool_sizes()
    assert len(pool) == 40 and len(set(pool)) == 40 and min(pool) == 1 and max(pool) == 640
    assert sorted(pool) == sorted(128 * (nt - 1) + r for nt in range(1, 6) for r in S.REMAINDERS)
    for nt in range(1, 6):                              # every last_pairs at every tile count, both sides of each pair edge
        mine = [n for n in pool if S.tiles(n) == nt]
        assert sorted(S.last_pairs(n) for n in mine) == [1, 1, 2, 2, 3, 3, 4, 4], nt
    assert [S.tiles(n) for n in S.deep_sizes()] == [12, 13]
    assert [S.last_pairs(n) for n in S.deep_sizes()] == [4, 1]
    # strips of the deep patches start at block rows 0, 2 .. 12, their second halves at 1, 3 .. 11
    assert sorted(2 * t.strip for t in S.tasks([S.deep_sizes()[1]])[0]) == list(range(0, 13, 2))
    fitted = S.fitted_pool_sizes()
    assert len(fitted) == 24 and set(fitted) <= set(pool) and 1 in fitted
    assert {S.tiles(n) for n in fitted} == {1, 2, 3, 4, 5} and {S.last_pairs(n) for n in fitted} == {1, 2, 3, 4}
    for name, idx in S.compositions(len(pool)).items():
        assert len(set(idx)) == len(idx) and len({S.tiles(pool[i]) for i in idx}) >= 4, name


def test_gpu_inputs_drive_the_branches_they_claim():
    batches = S.exact_batches(NUM_CU)
    hit = {name: S.branches(sizes, NUM_CU) for name, sizes in batches.items()}
    for name in ("pool", "reversed", "permuted"):
        assert hit[name] >= {"p_ge_8", "odd_nt", "even_nt", "half1_first_is_last", "nt_1", "last_pairs_1", "last_pairs_2",
                             "last_pairs_3", "last_pairs_4"}, name
        assert len(S.tasks(batches[name])[0]) == 72
    assert "p_lt_8" in hit["prefix7"] and "p_ge_8" in hit["prefix8"] and "p_ge_8" in hit["prefix9"]
    for name in ("deep12_alone", "deep13_alone"):
        assert hit[name] >= {"p_lt_8", "tasks_lt_8"}, name
    assert "even_nt" in hit["deep12_alone"] and "half1_first_is_last" in hit["deep12_alone"]
    assert "odd_nt" in hit["deep13_alone"] and "last_pairs_1" in hit["deep13_alone"]
    assert len(batches["deep12_and_seven_small"]) == 8
    assert hit["deep12_and_seven_small"] >= {"p_ge_8", "queue_longer_than_its_workgroups", "nt_1"}
    ts, off = S.tasks(batches["deep12_and_seven_small"])
    assert len(ts) == 13 and off[1] - off[0] == 6
    # more tasks than 1.5 times the workgroups, at this and at other CU counts
    for num_cu in (NUM_CU, 8, 64, 304):
        sizes = S.exact_batches(num_cu)["repeated"]
        assert len(S.tasks(sizes)[0]) >= 1.5 * num_cu and S.slots(sizes, num_cu) == num_cu
        assert "tasks_gt_slots" in S.branches(sizes, num_cu)
        fitted = S.fitted_pool_sizes()
        sizes = [fitted[i] for i in S.fitted_batches(num_cu)["repeated"]]
        assert len(S.tasks(sizes)[0]) >= 1.5 * num_cu and "tasks_gt_slots" in S.branches(sizes, num_cu)
    assert "tasks_gt_slots" in hit["repeated"] and "queue_longer_than_its_workgroups" in hit["repeated"]
    # the union is the full list
    cov = S.coverage(NUM_CU)
    assert sorted(cov) == sorted(S.BRANCHES), sorted(set(S.BRANCHES) - set(cov))
    assert set().union(*hit.values()) == set(S.BRANCHES)
