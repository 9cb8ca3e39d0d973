"""CPU tests of tests/_fit_schedule.py, the Python mirror of launch_cholesky / launch_split_solves: that the mirror is
self-consistent, that the inputs of tests/test_gpu_fit_schedule.py drive the schedule branches they are meant to drive
(at num_cu = 256, an MI355X), and that the number of K chunks never falls back to 1 once splitting has begun."""
import _fit_schedule as F

NUM_CU = 256


def test_pool_visits_every_residue_of_the_active_count():
    pool = F.pool_sizes()
    assert 38 <= len(pool) <= 42
    nts = [F.tiles(n) for n in pool]
    assert {1, 31, 32, 33, 127, 128, 129} <= set(pool)
    for e in range(1, 12):                                  # both sides of every tile edge up to 12 tiles
        assert 128 * e in pool and 128 * e + 1 in pool, e
    assert sum(nt > 20 for nt in nts) == 2 and len(set(pool)) < len(pool)
    s = F.schedule(pool, NUM_CU, 0)
    assert not s.split and s.solves == "backsolve" and all(L.nsplit == 1 for L in s.launches)
    assert {L.nactive % 8 for L in s.launches} == set(range(8))
    # the compositions: prefixes on both sides of 8 and 16 slots, every one ragged
    for name, idx in F.pool_compositions(len(pool)).items():
        assert sorted(set(idx)) == sorted(idx) and len({nts[i] for i in idx}) >= 5, name


def test_step_slot_deal_reaches_every_block_row_once():
    for nactive in range(1, 41):
        for G in (1, 2, 3, 7):
            got = sorted(F.step_slots(nactive, G).values())
            assert got == [(s, bx) for s in range(nactive) for bx in range(G)], (nactive, G)


def test_mirror_invariants_on_every_case():
    for name, sizes in list(F.edge_cases().items()) + [("pool", F.pool_sizes())]:
        for mode in (None, 0, 1, 2, 3):
            s = F.schedule(sizes, NUM_CU, mode)
            assert [L.l for L in s.launches] == list(range(s.max_nt - 1)), name       # no launch is skipped
            assert s.launches == [] or s.launches[-1].G == 1
            prev = None
            for L in s.launches:
                assert 1 <= L.nactive <= len(sizes) and L.G == s.max_nt - L.l - 1
                assert L.nactive == sum(nt >= s.max_nt - L.l for nt in s.nts)
                if prev is not None:
                    assert L.nactive >= prev.nactive                                  # patches enter, none leaves
                if L.nsplit > 1:
                    # the pending tiles are those of the split step just before, read from the OTHER half of the buffer
                    if prev is not None and prev.nsplit > 1:
                        assert L.pending == (prev.nactive, prev.G, 0 if prev.fold else prev.nsplit)
                        assert L.half != prev.half
                    else:
                        assert L.pending is None
                    assert L.nactive * (L.G + 1) * L.nsplit <= s.half_tiles
                    assert L.step_grid >= L.nactive * (L.G + (1 if L.fold else 0))
                    assert not (L.fold and L.G < 2)
                else:
                    assert L.pending is None and not L.fold
                prev = L
            assert (s.final_flush is not None) == bool(s.launches and s.launches[-1].nsplit > 1)
            if mode in (None, 0):
                assert not s.split or mode is None
            if mode == 2:
                assert s.solves == "blocks"
            if mode == 3:
                assert s.solves == "chained"


def test_edge_cases_cover_the_schedule_branches():
    cov = F.coverage(NUM_CU)
    for b in F.REQUIRED_BRANCHES:
        assert cov.get(b), (b, sorted(cov))
    # the case meant for each of the rarer branches
    assert "enter_after_split_12_7_6" in cov["pending launch with pend.n < nactive"]
    s = F.schedule(F.edge_cases()["enter_after_split_12_7_6"], NUM_CU, 1)
    assert [(L.l, L.nactive, L.nsplit) for L in s.launches[3:7]] == [(3, 1, 1), (4, 1, 2), (5, 2, 2), (6, 3, 3)]
    assert "ragged_40_2_1_39_17_1_6" in cov["nt = 1 patch in a split batch"]
    assert cov["solves by size: blocks"] == ["many_small_90x5_6_7"]
    assert "seven_large_26_25_24" in cov["fold on, and off at G = 1, in one fit"]
    assert "fold off with G >= 2" not in cov            # out of reach within 5200 points: see the test below
    # single patches of 2..5 tiles never split (l < 4): forced split mode runs the batched steps and the split solves
    for nt in (2, 3, 5):
        s = F.schedule([128 * nt], NUM_CU, 1)
        assert s.split and all(L.nsplit == 1 for L in s.launches) and s.final_flush is None and s.solves == "chained"
    # six tiles: exactly one split step, G = 1, no fold, flushed by the potrf-only launch with its partial sums
    s = F.schedule([768], NUM_CU, 1)
    assert [(L.l, L.nsplit, L.fold) for L in s.launches if L.nsplit > 1] == [(4, 2, False)] and s.final_flush == (1, 1, 2)
    # seven tiles: the first fold (l = 4, G = 2), then the G = 1 step whose partial launch factorises the folded tile
    s = F.schedule([896], NUM_CU, 1)
    assert [(L.l, L.G, L.nsplit, L.fold, L.pending) for L in s.launches if L.nsplit > 1] == \
        [(4, 2, 2, True, None), (5, 1, 2, False, (1, 2, 0))]
    # every patch of this file stays within 5200 points
    assert max(max(v) for v in F.edge_cases().values()) <= 5200


def test_chip_filling_bound_cannot_bind_below_67_tiles_at_256_cus():
    """nsplit_of's third term, (want_wg + G) / (G + 1), is below min(16, l / 2) only where G >= 34 and l >= 32: a patch of
    67 tiles (8449 points, a 570 MB slab).  The edge cases of the GPU file stay at 40 tiles, so at 256 CUs that term is
    checked on the mirror alone, here at a smaller num_cu, where the seven-patch case does drive it."""
    for max_nt in range(2, 67):
        s = F.schedule([128 * max_nt], NUM_CU, 1)
        assert "chip-filling bound on nsplit binds" not in F.branches(s), max_nt
    assert "chip-filling bound on nsplit binds" in F.branches(F.schedule([128 * 67], NUM_CU, 1))
    s = F.schedule(F.edge_cases()["seven_large_26_25_24"], 32, 1)
    assert "chip-filling bound on nsplit binds" in F.branches(s)
    # fold is switched off by G < 2 alone up to 64 tiles: (l + 1) <= 4 * nsplit_of(l + 1, G - 1) holds while l + 1 <= 64
    for max_nt in range(6, 65):
        s = F.schedule([128 * max_nt], NUM_CU, 1)
        assert all(L.fold == (L.G >= 2) for L in s.launches if L.nsplit > 1), max_nt
    assert "fold off with G >= 2" in F.branches(F.schedule([128 * 80], NUM_CU, 1))


def test_nsplit_never_falls_back_to_one():
    """Once a launch has split (nsplit > 1) every later launch of the fit splits too, for all max_nt <= 160 and P <= 64:
    the flush_pending() inside launch_cholesky's loop (the nsplit == 1 branch) never finds a pending tile, only the one
    after the loop does."""
    for num_cu in (NUM_CU, 304, 64):
        for max_nt in range(2, 161):
            ns = [F.nsplit_of(l, max_nt - l - 1, num_cu, True) for l in range(max_nt - 1)]
            assert ns == sorted(ns), (num_cu, max_nt)             # both of its terms grow with l (G shrinks)
            if num_cu >= NUM_CU:
                assert all(v > 1 for v in ns[4:]), (num_cu, max_nt)
    for max_nt in range(2, 161):
        for P in range(1, 65):
            # ragged: patches up to two tiles shorter than the largest
            sizes = [128 * max_nt] + [128 * max(1, max_nt - (r % 3)) for r in range(P - 1)]
            s = F.schedule(sizes, NUM_CU, 1)
            assert not any(L.flush_before for L in s.launches), (max_nt, P)
            split = [L.nsplit > 1 for L in s.launches]
            assert split == sorted(split), (max_nt, P)
