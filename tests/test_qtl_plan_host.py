"""CPU suite: what the QTL scan entry points plan on the host before they allocate (cnf2freq_amd/csrc/cnf2_qtlplan.h: the
marker map and the column tile), through cnf2h_qtl_marker_map and cnf2h_qtl_column_tile of the host library.  The expected
values are restated here in plain Python from the rules, not taken from the header; the tile rule is also held against the
seven expressions the entry points carried before they shared it."""
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


# ------------------------------------------------------------------------------------- 1. the marker map
def expected_map(cs, begin, end, tile, with_mchrom, whole):
    """The rules: the header (all chromstarts, or the first markers of the range's chromosomes); with_mchrom the chromosome
    of every marker of the map; a record {c, m, len, 0} per tile, the chromosomes of the range in order, each cut from its
    first marker on into tiles of `tile` markers with a shorter last one, c absolute under the whole-map header and relative
    to the range otherwise; the index of every chromosome's first tile, and the number of tiles behind them."""
    C = len(cs) - 1
    header = list(cs) if whole else list(cs[begin:end])
    mchrom = [c for c in range(C) for _ in range(cs[c], cs[c + 1])] if whole and with_mchrom else []
    tiles, tstart = [], [0]
    for c in range(begin, end):
        for m in range(cs[c], cs[c + 1], tile):
            tiles += [c if whole else c - begin, m, min(tile, cs[c + 1] - m), 0]
        tstart.append(len(tiles) // 4)
    return header + mchrom + tiles + tstart, len(header), len(header) + len(mchrom), len(header) + len(mchrom) + len(tiles)


def map_cases():
    for tile in (4, 16):
        # exactly one tile, one tile plus one marker, one marker, no marker, two tiles and a ragged third; then the lengths of
        # a whole tile plus a ragged one, an exact tile and a short one
        for lens in ((tile, tile + 1, 1, 0, 2 * tile + 3), (21, 16, 5), (0, 7), (5, 0)):
            cs = [0] + list(np.cumsum(lens))
            C = len(lens)
            for with_mchrom in (False, True):
                yield cs, 0, C, tile, with_mchrom, True
            for begin, end in ((1, C), (1, 2), (0, C), (C - 1, C)):
                yield cs, begin, end, tile, False, False                   # the sub-range form: first markers, relative c


def test_marker_map(host):
    n_cases = 0
    for cs, begin, end, tile, with_mchrom, whole in map_cases():
        got = host.qtl_marker_map(cs, tile, begin, end, with_mchrom=with_mchrom, whole_map_header=whole)
        want, o_mchrom, o_tiles, o_tstart = expected_map(cs, begin, end, tile, with_mchrom, whole)
        case = (cs, begin, end, tile, with_mchrom, whole)
        assert got["image"].dtype == np.int32 and got["image"].tolist() == want, case
        assert (got["o_mchrom"], got["o_tiles"], got["o_tstart"]) == (o_mchrom, o_tiles, o_tstart), case
        # the offsets as the callers use them
        C, M, nc = len(cs) - 1, cs[-1], end - begin
        if whole:
            assert got["o_mchrom"] == C + 1 and got["o_tiles"] == C + 1 + (M if with_mchrom else 0), case
            assert got["image"][:C + 1].tolist() == list(cs), case
        else:
            assert got["o_tiles"] == nc and got["image"][:nc].tolist() == list(cs[begin:end]), case
        assert got["o_tstart"] == got["o_tiles"] + 4 * got["n_tiles"], case
        assert len(got["image"]) == got["o_tstart"] + nc + 1, case
        tiles = got["image"][got["o_tiles"]:got["o_tstart"]].reshape(-1, 4)
        tstart = got["image"][got["o_tstart"]:]
        if whole and with_mchrom:
            mchrom = got["image"][got["o_mchrom"]:got["o_tiles"]]
            for m in range(M):
                assert cs[mchrom[m]] <= m < cs[mchrom[m] + 1], case
        # no tile straddles a start; the tiles cover every marker of the range once and in order
        covered = []
        for c, m, ln, pad in tiles:
            a = c if whole else c + begin
            assert pad == 0 and 1 <= ln <= tile and cs[a] <= m and m + ln <= cs[a + 1], case
            covered += range(m, m + ln)
        assert covered == list(range(cs[begin], cs[end])), case
        # tile_start[c + 1] - tile_start[c] = ceil(len_c / tile), and the tiles between them are that chromosome's
        assert tstart[0] == 0 and tstart[-1] == got["n_tiles"] == len(tiles), case
        for k, c in enumerate(range(begin, end)):
            assert tstart[k + 1] - tstart[k] == -(-(cs[c + 1] - cs[c]) // tile), case
            assert all(t[0] == (c if whole else k) for t in tiles[tstart[k]:tstart[k + 1]]), case
        n_cases += 1
    assert n_cases == 2 * 4 * 6
    with pytest.raises(ValueError):
        host.qtl_marker_map([0, 5, 9], 0)
    with pytest.raises(ValueError):
        host.qtl_marker_map([0, 5, 9], 4, 1, 3, whole_map_header=False)


# ------------------------------------------------------------------------------------- 2. the column tile
NSTAT, CHUNK = 5, 64            # QTLX_NSTAT (cnf2_qtlx.h), QTL2_CHUNK (cnf2_qtl2.h)


def expected_tile(n, R, P, per_column, cap):
    """The rule: the columns whose image [n][tile] of doubles stays under 1 GB, at least 16, at most 4096; with permutations
    the columns whose maxima (per_column doubles each; 0 = no such buffer) stay under 256 MB, at least 16; at most R; at most
    the cap where one is set."""
    rt = min(max(16, (1 << 30) // (8 * n)), 4096)
    if P > 0 and per_column > 0: rt = min(rt, max(16, (1 << 28) // (8 * per_column)))
    rt = min(rt, R)
    return min(rt, cap) if cap > 0 else rt


# The seven expressions of cnf2_capi.hip before the rule was shared, as Python one-liners (size_t division = //); x is what
# the scan sizes its maxima by.  Each with the per-column doubles it hands qtl_column_tile now.
_cap = lambda rt, cap: min(rt, cap) if cap > 0 else rt
_img = lambda n: max(16, (1 << 30) // (8 * n))
PARENT = {
    # qtl_scan_impl
    "scan": (lambda n, R, P, x, cap: _cap(min(min(_img(n), 4096), R), cap), lambda x: 0),
    # cnf2_qtl_scan_cols
    "cols": (lambda n, R, P, x, cap: _cap(min(min(_img(n), 4096), R), cap), lambda x: 0),
    # cnf2_qtl_scan2 (x = (L, n_chunks))
    "scan2": (lambda n, R, P, x, cap: _cap(min(min(min(_img(n), 4096), max(16, (1 << 28) // (24 * x[0] * x[1]))) if P > 0 else min(_img(n), 4096), R), cap),
              lambda x: 3 * x[0] * x[1]),
    # cnf2_qtl_scanx (x = n_tiles)
    "scanx": (lambda n, R, P, x, cap: _cap(min(min(min(_img(n), 4096), max(16, (1 << 28) // (8 * NSTAT * x))) if P > 0 else min(_img(n), 4096), R), cap),
              lambda x: NSTAT * x),
    # cnf2_qtl_scan_cof (x = n_tiles)
    "cof": (lambda n, R, P, x, cap: _cap(min(min(min(_img(n), 4096), max(16, (1 << 28) // (8 * x))) if P > 0 else min(_img(n), 4096), R), cap),
            lambda x: x),
    # cnf2_qtl_scan_em (x = n_tiles)
    "em": (lambda n, R, P, x, cap: _cap(min(min(min(_img(n), 4096), max(16, (1 << 28) // (8 * max(1, x)))) if P > 0 else min(_img(n), 4096), R), cap),
           lambda x: x),
    # cnf2_qtl_scan_binary (x = n_tiles)
    "binary": (lambda n, R, P, x, cap: _cap(min(min(min(_img(n), 4096), max(16, (1 << 28) // (8 * max(1, x)))) if P > 0 else min(_img(n), 4096), R), cap),
               lambda x: x),
}


def test_column_tile_each_term_binds(host):
    t = host.qtl_column_tile
    big = 10 ** 6
    assert t(100000, big, 0) == (1 << 30) // 800000 == 1342                      # the 1 GB image
    assert t(100, big, 0) == 4096                                                # the 4096
    assert t(100, big, 9, 50000) == (1 << 28) // 400000 == 671                   # the 256 MB of maxima
    assert t(100, 18, 9, 50000) == 18                                            # R
    assert t(100, 18, 9, 50000, 4) == 4                                          # the cap
    assert t(100, 18, 9, 50000, 40) == 18                                        # ... which only lowers
    assert t(100, 3, 9, 50000, 4) == 3
    assert t(2 * 10 ** 7, big, 0) == 16                                          # the floor of 16 under the image
    assert t(100, big, 9, 10 ** 7) == 16                                         # ... and under the maxima
    assert t(2 * 10 ** 7, 5, 0) == 5                                             # (R still lowers a floor)
    assert t(100, big, 0, 50000) == 4096                                         # P = 0: the maxima bound is off
    assert t(100, big, 9, 0) == 4096                                             # no per-column doubles: no such bound
    assert t(100, big, 9, 1) == 4096
    for bad in ((-1, 5, 0, 0, 0), (5, 5, 0, 0, -1), (5, 5, 0, -2, 0)):
        with pytest.raises(ValueError):
            t(*bad)


def test_column_tile_is_what_the_seven_entry_points_computed(host):
    ns = (1, 24, 1000, 32767, 32768, 32769, 100000, 2 ** 23, 2 ** 23 + 1, 2 * 10 ** 7)
    Rs = (1, 3, 18, 4095, 4096, 4097, 10 ** 6)
    caps = (0, 1, 4, 16, 5000)
    n_tiles = (0, 1, 3, 400, 8191, 8192, 8193, 50000, 2 ** 21, 2 ** 21 + 1, 10 ** 7)
    pairs = [(L, -(-(L - 1) // CHUNK)) for L in (2, 64, 65, 66, 700, 4096)]
    n_checked = 0
    for name, (parent, per_column) in PARENT.items():
        xs = pairs if name == "scan2" else n_tiles if name in ("em", "binary") else (0,) if name in ("scan", "cols") else n_tiles[1:]
        for n, R, P, x, cap in itertools.product(ns, Rs, (0, 1, 1000), xs, caps):
            want = parent(n, R, P, x, cap)
            assert want == expected_tile(n, R, P, per_column(x), cap), (name, n, R, P, x, cap)
            assert host.qtl_column_tile(n, R, P, per_column(x), cap) == want, (name, n, R, P, x, cap)
            n_checked += 1
    assert n_checked > 30000
