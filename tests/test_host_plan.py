"""CPU suite: the sweep entry points' planner (cnf2freq_amd/csrc/cnf2_plan.h: job list, grids and spill, batches) compiled
for the host.  The expected values are restated here in plain Python from the rules, not taken from the planner."""
import ctypes as C

import numpy as np
import pytest

from cnf2freq_amd import capi
from conftest import load_trajectory

# the 64-byte window record (cnf2_window.h) and the slot flags (cnf2_emission.h)
WINDOW = np.dtype({"names": ["row", "flags", "tie", "shiftignore", "shiftend", "n_groups", "flag2ignore", "rec"],
                   "formats": [("<i4", 7), ("u1", 7), ("i1", 7), "u1", "u1", "u1", "u1", "<i4"],
                   "offsets": [0, 28, 35, 42, 43, 44, 45, 48], "itemsize": 64})
PRESENT, FOUNDER, HOM = 1, 2, 8
WAVES = 4                 # wavefronts per block
SPILL_ROW = 528           # doubles of a spill slot per marker
FITS, NO_SPILL, NO_PART, NO_ROWS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def shim():
    from conftest import build_host_shim
    s = build_host_shim()
    U64 = C.c_uint64
    s.shim_windows.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    s.shim_windows.restype = None
    s.shim_plan_jobs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 5
    s.shim_plan_sweep_grids.argtypes = [C.c_int] * 4 + [U64] * 4 + [C.c_int, C.c_void_p]
    s.shim_plan_batches.argtypes = [C.c_int] * 3 + [U64, U64, C.c_int, U64, U64, C.c_int, U64, U64, C.c_void_p]
    s.shim_plan_batches.restype = None
    s.shim_whole_rounds.argtypes = [U64, U64, C.c_int]
    s.shim_whole_rounds.restype = U64
    return s


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def windows_of(shim, ped, row_hom=None):
    out = np.zeros(len(ped.dous), WINDOW)
    dous = np.ascontiguousarray(ped.dous, np.int32)
    shim.shim_windows(ped.n_rec, _p(ped.par), _p(ped.empty), _p(ped.gen), _p(ped.row_of), _p(dous), len(dous),
                      None if row_hom is None else _p(row_hom), 0 if row_hom is None else len(row_hom), _p(out))
    return out


def plan_jobs(shim, win, chromstarts, ind_begin, n, flags, row_hom):
    cs = np.ascontiguousarray(chromstarts, np.int32)
    C_ = len(cs) - 1
    jobs, pjobs = np.full((n * C_ + 1, 4), -9, np.int32), np.full((n * C_ + 1, 8), -9, np.int32)
    n_fast, n_pj = np.zeros(1, np.int32), np.zeros(1, np.int32)
    nj = shim.shim_plan_jobs(_p(win), _p(cs), C_, ind_begin, n, flags, _p(row_hom), _p(jobs), _p(n_fast), _p(pjobs), _p(n_pj))
    return jobs[:nj].tolist(), int(n_fast[0]), pjobs[:n_pj[0]].tolist()


def expected_jobs(win, chromstarts, ind_begin, n, flags, row_hom):
    """The rules: untied windows' jobs first, then the tied ones'; within each the chromosomes longest first (equal lengths in
    map order) and the individuals ascending.  CNF2_NO_TIES: no window is tied; CNF2_FLUSH_TINY: every window is.  Under
    CNF2_MERGE_MODES (not with CNF2_FULL_SPILL or CNF2_FLUSH_TINY) windows that are not tied, analyse all 8 shift modes, are
    not the top of their lines and have both parents present on rows that are homozygous everywhere leave the list in groups
    of four per class (class 1: all four grandparents present and homozygous everywhere); what does not fill a group stays."""
    lens = np.diff(chromstarts)
    order = sorted(range(len(lens)), key=lambda c: -lens[c])
    w = win[ind_begin:ind_begin + n]
    active = [bool(x["n_groups"] > 0 and not flags & capi.NO_TIES) for x in w]
    tied = [bool(a or flags & capi.FLUSH_TINY) for a in active]
    packed, pjobs = set(), []
    if flags & capi.MERGE_MODES and not flags & (capi.FULL_SPILL | capi.FLUSH_TINY):
        def mergeable(j):
            x = w[j]
            parents_hom = all(x["flags"][k] & PRESENT and x["row"][k] >= 0 and row_hom[x["row"][k]] for k in (1, 4))
            return not active[j] and x["shiftignore"] == 0 and x["shiftend"] == 8 and not x["flags"][0] & FOUNDER and parents_hom
        for cls in (0, 1):
            el = [j for j in range(n) if mergeable(j)
                  and int(all(w[j]["flags"][k] & PRESENT and w[j]["flags"][k] & HOM for k in (2, 3, 5, 6))) == cls]
            groups = [el[k:k + 4] for k in range(0, len(el) - len(el) % 4, 4)]
            packed.update(j for g in groups for j in g)
            pjobs += [g + [int(chromstarts[c]), int(chromstarts[c + 1]) - 1, c, cls] for c in order for g in groups]
    jobs = [[j, int(chromstarts[c]), int(chromstarts[c + 1]) - 1, c]
            for want_tied in (False, True) for c in order for j in range(n) if j not in packed and tied[j] == want_tied]
    return jobs, sum(1 for j in range(n) if j not in packed and not tied[j]) * len(lens), pjobs


@pytest.mark.parametrize("case, chromstarts", [("ail_ties", [0, 3, 8, 11, 16, 18]), ("ail_ties", None),
                                               ("outbred3_two_chrom", None), ("outbred3_two_chrom", [0, 4, 4 + 9, 20])])
@pytest.mark.parametrize("flags", [0, capi.NO_TIES, capi.FLUSH_TINY, capi.NO_TIES | capi.FLUSH_TINY])
def test_job_order(shim, case, chromstarts, flags):
    ped, _, _ = load_trajectory(case)
    cs = np.asarray(ped.chromstarts if chromstarts is None else chromstarts, np.int32)
    win = windows_of(shim, ped)
    row_hom = np.zeros(int(ped.row_of.max()) + 1, np.uint8)
    if case == "ail_ties": assert (win["n_groups"] > 0).any() and (win["n_groups"] == 0).any()
    for ind_begin, n in [(0, len(win)), (2, len(win) - 3), (1, 1)]:
        jobs, n_fast, pjobs = plan_jobs(shim, win, cs, ind_begin, n, flags, row_hom)
        want, want_fast, _ = expected_jobs(win, cs, ind_begin, n, flags, row_hom)
        assert jobs == want and n_fast == want_fast and pjobs == []
        assert len(jobs) == n * (len(cs) - 1)
        if flags & capi.FLUSH_TINY: assert n_fast == 0            # every window in the second list
        elif flags & capi.NO_TIES: assert n_fast == len(jobs)     # every window in the first
        lens = [j[2] - j[1] + 1 for j in jobs]
        for part in (lens[:n_fast], lens[n_fast:]):
            assert part == sorted(part, reverse=True)             # longest chromosome first


def fabricated_windows(seed, n):
    """Windows with every combination the packing rule looks at; rows 0..9, of which the even ones are homozygous everywhere."""
    rng = np.random.default_rng(seed)
    win = np.zeros(n, WINDOW)
    win["row"] = rng.integers(-1, 10, (n, 7))
    win["flags"] = rng.choice([PRESENT, PRESENT | HOM, PRESENT | HOM, 0, PRESENT | FOUNDER], (n, 7))
    win["flags"][:, 0] = rng.choice([PRESENT, PRESENT, PRESENT, PRESENT | FOUNDER], n)
    easy = rng.random(n) < 0.75                  # a good share of windows that do qualify
    win["flags"][easy, 1] = win["flags"][easy, 4] = PRESENT | HOM
    win["row"][easy, 1], win["row"][easy, 4] = 2, 4
    leaf = rng.random(n) < 0.5                   # ... and of windows whose grandparents are all homozygous everywhere
    for k in (2, 3, 5, 6): win["flags"][leaf, k] = PRESENT | HOM
    win["n_groups"] = rng.choice([0, 0, 0, 0, 1, 2], n)
    win["shiftignore"] = rng.choice([0, 0, 0, 0, 2], n)
    win["shiftend"] = rng.choice([8, 8, 8, 2], n)
    return win, (np.arange(10) % 2 == 0).astype(np.uint8)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("extra", [0, capi.NO_TIES, capi.FULL_SPILL, capi.FLUSH_TINY])
def test_packing_under_merge_modes(shim, seed, extra):
    n_all = 120
    win, row_hom = fabricated_windows(seed, n_all)
    cs = np.array([0, 5, 17, 22, 34, 36], np.int32)
    flags = capi.MERGE_MODES | extra
    for ind_begin, n in [(0, n_all), (3, 90)]:
        jobs, n_fast, pjobs = plan_jobs(shim, win, cs, ind_begin, n, flags, row_hom)
        want, want_fast, want_p = expected_jobs(win, cs, ind_begin, n, flags, row_hom)
        assert jobs == want and n_fast == want_fast and pjobs == want_p
        in_packed = {j for pj in pjobs for j in pj[:4]}
        assert not in_packed & {j[0] for j in jobs}               # no individual in both lists
        assert len(jobs) + 4 * len(pjobs) == n * (len(cs) - 1)
        if extra in (0, capi.NO_TIES):
            assert pjobs and {pj[7] for pj in pjobs} == {0, 1}    # both classes occur in the fabricated set
            for cls in (0, 1):                                    # fewer than four of a class are left over
                assert sum(1 for j in range(n) if j not in in_packed and _class_of(win[ind_begin + j], row_hom, flags) == cls) < 4
        else: assert pjobs == []


def _class_of(x, row_hom, flags):
    """-1: not mergeable; else the homleaf class (restated once more, for the leftover count)."""
    if (x["n_groups"] > 0 and not flags & capi.NO_TIES) or x["shiftignore"] or x["shiftend"] != 8 or x["flags"][0] & FOUNDER:
        return -1
    if not all(x["flags"][k] & PRESENT and x["row"][k] >= 0 and row_hom[x["row"][k]] for k in (1, 4)):
        return -1
    return int(all(x["flags"][k] & (PRESENT | HOM) == PRESENT | HOM for k in (2, 3, 5, 6)))


def expected_grids(n_cu, fast_per_cu, gen_per_cu, reserve, n_fast, n_general, free, held, max_len):
    """One wave per job, at most the resident blocks less the reserve (at least one); the spill slots of all blocks -- 4 waves x
    max_len x 528 doubles each -- stay within 60 % of free + held: each grid alone, and their sum when both kernels run (then
    blocks are taken off the fast grid and the general grid in turn, never below one each)."""
    budget = int(float(free + held) * 0.6)
    per_blk = WAVES * max_len * SPILL_ROW * 8
    if budget // per_blk < 1: return None
    grid = lambda nj, per_cu: min(-(-nj // WAVES), max(1, n_cu * per_cu - reserve), budget // per_blk)
    gf, gg = grid(n_fast, fast_per_cu), grid(n_general, gen_per_cu)
    if n_fast and n_general:
        while (gf + gg) * per_blk > budget and gf + gg > 2:
            if gf > 1: gf -= 1
            if gg > 1 and (gf + gg) * per_blk > budget: gg -= 1
    return gf, gg


def test_sweep_grids_and_spill(shim):
    rng = np.random.default_rng(5)
    per_blk = lambda max_len: WAVES * max_len * SPILL_ROW * 8
    cases = [(256, 2, 1, 0, 100000, 5000, 200 << 30, 0, 400),        # memory is no limit: the resident blocks
             (256, 2, 1, 8, 100000, 5000, 200 << 30, 0, 400),        # ... less the reserve
             (256, 2, 1, 0, 37, 5, 200 << 30, 0, 400),               # few jobs: one wave per job
             (256, 2, 1, 0, 100000, 0, 200 << 30, 0, 400),           # one kernel only
             (256, 2, 1, 0, 0, 7000, 200 << 30, 0, 400),
             (256, 2, 1, 0, 100000, 5000, 3 << 30, 1 << 30, 20000),  # the budget binds, held memory counts
             (4, 1, 1, 100, 1000, 1000, 1 << 30, 0, 100),            # the reserve exceeds the machine: one block each
             (256, 2, 1, 0, 100000, 5000, int(per_blk(50000) / 0.6) + 4096, 0, 50000),   # exactly one block fits
             (256, 2, 1, 0, 100000, 5000, int(per_blk(50000) * 2 / 0.6) + 4096, 0, 50000)]
    for _ in range(200):
        cases.append((int(rng.integers(1, 305)), int(rng.integers(1, 4)), int(rng.integers(1, 3)), int(rng.integers(0, 40)),
                      int(rng.integers(0, 3000)), int(rng.integers(0, 3000)), int(rng.integers(1 << 20, 1 << 34)),
                      int(rng.integers(0, 1 << 30)), int(rng.integers(1, 30000))))
    seen_shared = 0
    for c in cases:
        g = np.zeros(2, np.int32)
        ok = shim.shim_plan_sweep_grids(*c, _p(g))
        want = expected_grids(*c)
        assert bool(ok) == (want is not None), c
        if want is None: continue
        assert tuple(g) == want, c
        n_cu, fast_per_cu, gen_per_cu, reserve, n_fast, n_general, free, held, max_len = c
        budget = int(float(free + held) * 0.6)
        assert (g[0] > 0) == (n_fast > 0) and (g[1] > 0) == (n_general > 0)
        if n_fast and n_general and g[0] + g[1] > 2:
            assert (int(g[0]) + int(g[1])) * per_blk(max_len) <= budget, c       # both run: their slots fit the 60 % together
            seen_shared += (-(-n_fast // WAVES) + -(-n_general // WAVES)) * per_blk(max_len) > budget
    assert seen_shared > 20
    # not even one block fits
    g = np.zeros(2, np.int32)
    assert shim.shim_plan_sweep_grids(256, 2, 1, 0, 1000, 1000, int(per_blk(50000) / 0.6) - 4096, 0, 50000, _p(g)) == 0
    assert shim.shim_plan_sweep_grids(256, 2, 1, 0, 1000, 1000, int(per_blk(50000) / 0.6) - 4096, 8192, 50000, _p(g)) == 1


def expected_whole_rounds(batch, n_jobs, grid_cap):
    waves = grid_cap * WAVES
    return batch if batch >= n_jobs or batch < waves else batch // waves * waves


def expected_batches(n_cu, per_cu, reserve, free, held, max_len, row_doubles, n_jobs, batch_jobs, part_need, part_held):
    """Spill: the resident blocks' slots, at most a quarter of free + held.  CNF2_DETERMINISTIC rows (part_need doubles, part_held
    of them held already): must fit half of it, and what has to be newly allocated is taken out first.  Batch: the jobs whose
    rows (max_len x row_doubles doubles each) fit half of the rest after the spill; at most all jobs and 1 000 000; a whole
    number of rounds of the resident waves; at most batch_jobs if that is set."""
    free += held
    per_blk = WAVES * max_len * SPILL_ROW * 8
    grid_cap = min(max(1, n_cu * per_cu - reserve), free // 4 // per_blk)
    if grid_cap < 1: return NO_SPILL, None, None
    if part_need:
        if part_need * 8 > free // 2 + part_held * 8: return NO_PART, grid_cap, None
        free -= max(0, part_need * 8 - part_held * 8)
    batch = (free - grid_cap * per_blk) // 2 // (max_len * row_doubles * 8)
    if batch < 1: return NO_ROWS, grid_cap, None
    batch = expected_whole_rounds(min(batch, n_jobs, 1000000), n_jobs, grid_cap)
    if batch_jobs > 0: batch = min(batch, batch_jobs)
    return FITS, grid_cap, batch


def test_whole_rounds(shim):
    for batch, n_jobs, grid_cap in [(5000, 5000, 256), (6000, 5000, 256), (1000, 5000, 256), (1023, 5000, 256), (1024, 5000, 256),
                                    (1025, 5000, 256), (4999, 5000, 256), (2047, 9000, 256), (7, 9, 1), (3, 9, 1)]:
        assert shim.shim_whole_rounds(batch, n_jobs, grid_cap) == expected_whole_rounds(batch, n_jobs, grid_cap)
    assert shim.shim_whole_rounds(6000, 5000, 256) == 6000         # covers all jobs: unchanged
    assert shim.shim_whole_rounds(1000, 5000, 256) == 1000         # less than one round of 1 024 waves: unchanged
    assert shim.shim_whole_rounds(4999, 5000, 256) == 4096


def test_batches(shim):
    def run(*c):
        out = np.full(3, -7, np.int64)
        shim.shim_plan_batches(*c, _p(out))
        want = expected_batches(*c)
        assert out[0] == want[0], c
        if want[0] != NO_SPILL: assert out[1] == want[1], c
        if want[0] == FITS: assert out[2] == want[2], c
        return out
    GB = 1 << 30
    # (n_cu, per_cu, reserve, free, held, max_len, row_doubles, n_jobs, batch_jobs, part_need, part_held)
    o = run(256, 2, 0, 200 * GB, 0, 1000, 512, 50000, 0, 0, 0)
    assert o[1] == 512 and o[2] == (200 * GB - 512 * WAVES * 1000 * SPILL_ROW * 8) // 2 // (1000 * 512 * 8) // 2048 * 2048
    o = run(256, 2, 0, 8 * GB, 0, 1000, 512, 50000, 0, 0, 0)             # the quarter binds: fewer blocks
    assert o[1] == 8 * GB // 4 // (WAVES * 1000 * SPILL_ROW * 8) < 512
    assert run(256, 2, 0, 6 * GB, 2 * GB, 1000, 512, 50000, 0, 0, 0).tolist() == o.tolist()     # held memory counts as free
    assert run(256, 2, 0, 200 * GB, 0, 10, 512, 3000000, 0, 0, 0)[2] == 1000000 // 2048 * 2048  # the cap of 1 000 000
    assert run(256, 2, 0, 200 * GB, 0, 1000, 512, 300, 0, 0, 0)[2] == 300                       # all jobs in one batch
    assert run(256, 2, 0, 200 * GB, 0, 1000, 512, 50000, 777, 0, 0)[2] == 777                   # batch_jobs, after the rounding
    assert run(256, 2, 0, 200 * GB, 0, 1000, 1056, 50000, 0, 0, 0)[2] == \
        (200 * GB - 512 * WAVES * 1000 * SPILL_ROW * 8) // 2 // (1000 * 1056 * 8) // 2048 * 2048
    # part_need comes out before the batch is sized; what is held of it does not
    base = run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 0, 0)
    part = run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 2 * GB, 0)    # 16 GB of rows
    assert part[1] == base[1] and part[2] == (48 * GB - int(base[1]) * WAVES * 1000 * SPILL_ROW * 8) // 2 // (1000 * 512 * 8) // 2048 * 2048
    assert part[2] < base[2]
    assert run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 2 * GB, 2 * GB)[2] == base[2]
    assert run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 2 * GB, GB)[2] > part[2]
    # what does not fit
    assert run(256, 2, 0, 60 << 20, 0, 1000, 512, 50000, 0, 0, 0)[0] == NO_SPILL
    assert run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 4 * GB + 1, 0)[0] == NO_PART          # more than half
    assert run(256, 2, 0, 64 * GB, 0, 1000, 512, 50000, 0, 4 * GB, 0)[0] == FITS
    assert run(1, 1, 0, 400 << 20, 0, 5000, 100000, 50000, 0, 0, 0)[0] == NO_ROWS         # (rows far wider than the two in use)
    rng = np.random.default_rng(11)
    fits = 0
    for _ in range(300):
        need = int(rng.integers(0, 1 << 28)) * int(rng.integers(0, 2))
        fits += run(int(rng.integers(1, 305)), int(rng.integers(1, 4)), int(rng.integers(0, 40)), int(rng.integers(1 << 24, 1 << 36)),
                    int(rng.integers(0, 1 << 31)), int(rng.integers(1, 20000)), int(rng.choice([512, 1056])),
                    int(rng.integers(1, 2000000)), int(rng.integers(0, 3)) * int(rng.integers(1, 5000)), need,
                    int(rng.integers(0, need + 1)))[0] == FITS
    assert 100 < fits < 300


def test_job_order_of_the_persistent_mode_fixtures(shim):
    """tests/test_gpu_persistent_modes.py works out which wave of one block takes which job from its own statement of the job
    order (job_lists): for each of its fixtures that statement is the planner's list, with the tie rule (the modes) and without
    (the placement sweep)"""
    import test_gpu_persistent_modes as pm
    for name in pm.FIXTURES:
        fx = pm.fixture(name)
        ped = fx.ped
        row_hom = ((ped.allele[:, :, 0] == ped.allele[:, :, 1]) & (ped.sure[:, :, 0] == ped.sure[:, :, 1])).all(axis=1).astype(np.uint8)
        win = windows_of(shim, ped, row_hom)
        for flags in (0, capi.NO_TIES):
            tied = (win["n_groups"] > 0) & (flags == 0)
            paths = np.where(tied, pm.PATH_TIED, 0)[:, None].repeat(fx.C, axis=1)
            untied, tied_jobs = pm.job_lists(fx, paths)
            jobs, n_fast, pjobs = plan_jobs(shim, win, ped.chromstarts, 0, fx.n, flags, row_hom)
            assert [(j[0], j[3]) for j in jobs] == untied + tied_jobs and n_fast == len(untied) and pjobs == []
        assert (len(tied_jobs) == 0) and (win["n_groups"] > 0).sum() * fx.C == (70 if name == "tied_mixed" else 0)
