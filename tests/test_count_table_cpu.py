"""The CPU statement of the u8 count table (oracle/count_table_oracle.py) and the case table of tests/test_count_table_gpu.py.

* Layout: `encode` against a literal per-byte loop over the index formula of thermoextrap_amd/csrc/txm_i8g.h -- the loop
  splits every byte offset into (g, t, s, q, L, b) with integer division and looks the count up; it shares no reshape with
  `encode`.
* Round trip: `decode(encode(f))` gives the live rows back and zeros elsewhere.
* The case table: what the GPU module assumes about its cases is proved here from the CPU restatement of the sampler
  stream (`orc.sampler_tile_counts` / `orc.sampler_freq`) and from restated rules of txm_count_table.hip -- every count
  fits a byte, every half group of every slab takes the path its case is named for, the table as a whole reaches every
  path, both tile kinds and all three Philox loops of the full-tile path, and some (replicate, tile) draws nothing.
"""

import numpy as np
import pytest

from oracle import count_table_oracle as cto

TILE, GROUP, HALF = 1024, 128, 64
LABELS = ("full", "dead lanes", "pack 2", "pack 4", "pack 8", "dead half")


# ---- restated rules of txm_count_table.hip -----------------------------------------------------------------------------
def half_label(live):
    """Path of a 64-replicate half group with `live = nrep - rep_begin - 64 h` replicates of the call in it."""
    if live >= 64:
        return "full"
    if live >= 33:
        return "dead lanes"
    if live >= 17:
        return "pack 2"
    if live >= 9:
        return "pack 4"
    if live >= 1:
        return "pack 8"
    return "dead half"


def half_labels(nrep, rep_begin, nreps):
    groups = -(-nreps // GROUP)
    return tuple(half_label(nrep - rep_begin - HALF * h) for h in range(2 * groups))


def tile_kinds(N):
    """("full", ...) and, for a ragged N, ("partial", shift): the last tile's window slides back by `shift` samples."""
    nt = -(-N // TILE)
    last = N - TILE * (nt - 1)
    kinds = {"full"} if nt > 1 or last == TILE else set()
    shift = TILE * (nt - 1) - min(TILE * (nt - 1), N - TILE)
    if last < TILE:
        kinds.add("partial")
    return kinds, shift


def philox_loops(nmin, nmax, waves=8):
    """Loops of the lane-per-replicate fill that some wave enters for a full tile whose live lanes draw nmin .. nmax times:
    calls below nmin // 12 are complete for every lane ("two chains" while two of a wave's calls fit, then "one chain"),
    the rest up to the last call of the busiest lane are "ragged"."""
    call_all, hit = nmin // 12, set()
    for w in range(waves):
        c = w
        while c + waves < call_all:
            hit.add("two chains")
            c += 2 * waves
        while c < call_all:
            hit.add("one chain")
            c += waves
        if c * 12 < nmax:
            hit.add("ragged")
    return hit


# ---- the case table of group A (tests/test_count_table_gpu.py) ----------------------------------------------------------
SEED = 0x9E3779B97F4A7C15      # every case: a non-zero high seed word


def case(id, N, nrep, halves, *, nsamp=0, rep0=0, slab=None, k=0):
    rb, nr = slab or (0, nrep)
    return dict(id=id, seed=SEED + 0x100000001 * k, N=N, nrep=nrep, nsamp=nsamp, rep0=rep0, rep_begin=rb, nreps=nr, halves=halves)


_F, _DL, _P2, _P4, _P8, _DH = LABELS
_N2047 = {1: (_P8, _DH), 8: (_P8, _DH), 9: (_P4, _DH), 16: (_P4, _DH), 17: (_P2, _DH), 32: (_P2, _DH), 33: (_DL, _DH), 63: (_DL, _DH),
          64: (_F, _DH), 65: (_F, _P8), 72: (_F, _P8), 73: (_F, _P4), 80: (_F, _P4), 81: (_F, _P2), 96: (_F, _P2), 97: (_F, _DL),
          127: (_F, _DL), 128: (_F, _F), 129: (_F, _F, _P8, _DH)}
_TOP = 2**32 - 330             # the last 330 replicates of the stream range
GROUP_A = (
    [case("N1024-r64", 1024, 64, (_F, _DH), k=1),                                  # one full tile, no slide
     case("N1025-r130", 1025, 130, (_F, _F, _P8, _DH), k=2)]                       # a last tile of one sample, shift 1023
    + [case(f"N2047-r{r}", 2047, r, h, k=3) for r, h in _N2047.items()]            # both sides of every fill-width boundary
    + [case("N5000-r330-top", 5000, 330, (_F,) * 5 + (_P4,), rep0=_TOP, k=4),
       case("N5000-r330-top-from128", 5000, 330, (_F, _F, _F, _P4), rep0=_TOP, slab=(128, 202), k=4),
       case("N5000-r330-top-from256", 5000, 330, (_F, _P4), rep0=_TOP, slab=(256, 74), k=4),
       case("N5000-r330-top-group1", 5000, 330, (_F, _F), rep0=_TOP, slab=(128, 72), k=4),      # one whole group, all of it live
       case("N5000-r330-top-past-nrep", 5000, 330, (_F, _P4) + (_DH,) * 4, rep0=_TOP, slab=(256, 300), k=4),   # two groups all zero
       case("N2047-r8-dense", 2047, 8, (_P8, _DH), nsamp=16 * 2047, k=5),           # mean 16 per sample
       case("N3000-r40-sparse", 3000, 40, (_DL, _DH), nsamp=1000, k=6),             # few draws per tile, dead lanes
       case("N3000-r100-nsamp5", 3000, 100, (_F, _DL), nsamp=5, k=7),               # most tiles empty: ragged loop only
       case("N4096-r72-nsamp8192", 4096, 72, (_F, _P8), nsamp=8192, k=8)]           # no partial tile
)


def reference(orc, c):
    """(tile counts, frequency rows) of the case's call from the CPU restatement of the stream."""
    counts = orc.sampler_tile_counts(c["seed"], c["nrep"], c["N"], c["nsamp"], rep0=c["rep0"])
    return counts, orc.sampler_freq(c["seed"], c["nrep"], c["N"], c["nsamp"], counts=counts, rep0=c["rep0"])


_REF = {}


def cached_reference(orc, c):
    key = (c["seed"], c["nrep"], c["N"], c["nsamp"], c["rep0"])
    if key not in _REF:
        _REF[key] = reference(orc, c)
    return _REF[key]


# ---- layout ------------------------------------------------------------------------------------------------------------
def literal_table(freq, N, nrep, rep_begin, nreps):
    """txm_i8g.h's formula, one byte at a time."""
    nt = -(-N // TILE)
    nbytes = -(-nreps // GROUP) * nt * TILE * GROUP
    out = np.empty(nbytes, dtype=np.uint8)
    for i in range(nbytes):
        b, L, q, s = i % 16, (i // 16) % 64, (i // 1024) % 4, (i // 4096) % 32
        t, g = (i // 131072) % nt, i // (131072 * nt)
        sample = min(1024 * t, N - 1024) + 32 * s + 16 * (L >> 5) + b
        rep = rep_begin + 128 * g + 32 * q + (L & 31)
        foreign = sample < 1024 * t                 # the slid last tile: samples of the tile before it
        out[i] = 0 if (rep >= nrep or foreign) else freq[rep, sample]
    return out


@pytest.mark.parametrize("N,nrep,rep_begin,nreps", [(1024, 100, 0, 100), (1025, 300, 128, 140)])
def test_encode_is_the_headers_formula_byte_by_byte(N, nrep, rep_begin, nreps):
    freq = np.random.default_rng(N).integers(0, 256, size=(nrep, N))
    got = cto.encode(freq, N, nrep, rep_begin, nreps)
    assert got.dtype == np.uint8 and got.shape == (cto.count_table_bytes(N, nreps),)
    assert got.shape[0] == -(-nreps // 128) * -(-N // 1024) * 131072
    assert np.array_equal(got, literal_table(freq, N, nrep, rep_begin, nreps))


@pytest.mark.parametrize("N,nrep,rep_begin,nreps", [
    (1024, 64, 0, 64), (1025, 130, 0, 130), (2047, 129, 128, 1), (5000, 330, 128, 72), (5000, 330, 256, 300), (4096, 72, 0, 72)])
def test_decode_undoes_encode(N, nrep, rep_begin, nreps):
    freq = np.random.default_rng(nrep).integers(0, 256, size=(nrep, N))
    rows = cto.decode(cto.encode(freq, N, nrep, rep_begin, nreps), N, nreps)
    live = min(nrep - rep_begin, rows.shape[0])
    assert rows.dtype == np.int64 and rows.shape == (-(-nreps // 128) * 128, N)
    assert np.array_equal(rows[:live], freq[rep_begin:rep_begin + live])
    assert not rows[live:].any()


def test_encode_refuses_what_the_entry_point_refuses():
    freq = np.zeros((130, 2048), dtype=np.int64)
    for rb, nr in ((64, 10), (256, 10), (0, 0), (-128, 10)):
        with pytest.raises(ValueError):
            cto.encode(freq, 2048, 130, rb, nr)
    with pytest.raises(ValueError):
        cto.encode(freq[:, :1023], 1023, 130, 0, 130)
    freq[129, 2047] = 256
    cto.encode(freq, 2048, 130, 0, 128)             # the row is outside the slab
    with pytest.raises(ValueError):
        cto.encode(freq, 2048, 130, 128, 2)
    assert cto.count_table_bytes(1023, 5) == 0 and cto.count_table_bytes(5000, 0) == 0
    assert cto.count_table_bytes(1025, 129) == 2 * 2 * 131072


# ---- the case table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUP_A, ids=[c["id"] for c in GROUP_A])
def test_case_is_what_it_is_named_for(orc, c):
    assert c["seed"] >> 32 and c["rep_begin"] % GROUP == 0 and 0 <= c["rep_begin"] < c["nrep"] and c["nreps"] >= 1
    assert 0 <= c["rep0"] and c["rep0"] + c["nrep"] <= 2**32
    assert half_labels(c["nrep"], c["rep_begin"], c["nreps"]) == c["halves"]
    counts, freq = cached_reference(orc, c)
    assert freq.min() >= 0 and freq.max() <= 255
    assert np.all(freq.sum(axis=1) == (c["nsamp"] or c["N"]))
    table = cto.encode(freq, c["N"], c["nrep"], c["rep_begin"], c["nreps"])
    live = min(c["nrep"] - c["rep_begin"], -(-c["nreps"] // GROUP) * GROUP)
    assert int(table.astype(np.int64).sum()) == live * (c["nsamp"] or c["N"])


def test_case_table_reaches_every_path(orc):
    by_id = {c["id"]: c for c in GROUP_A}
    assert len(by_id) == len(GROUP_A)
    assert {lab for c in GROUP_A for lab in c["halves"]} == set(LABELS)
    # every fill width on either side of its boundary, in the first half group and in the second
    for first, second in ((8, 9), (16, 17), (32, 33), (63, 64)):
        for off in (0, 64):
            a, b = by_id[f"N2047-r{first + off}"], by_id[f"N2047-r{second + off}"]
            assert a["halves"][off // 64] != b["halves"][off // 64]
    kinds, shifts = set(), set()
    for c in GROUP_A:
        k, shift = tile_kinds(c["N"])
        kinds |= k
        shifts.add(shift)
    assert kinds == {"full", "partial"} and {0, 1, 120, 1023} <= shifts
    assert tile_kinds(1024) == ({"full"}, 0) and tile_kinds(4096) == ({"full"}, 0)       # no slide, no partial tile
    assert tile_kinds(1025) == ({"full", "partial"}, 1023) and tile_kinds(2047) == ({"full", "partial"}, 1)
    # the three Philox loops of the lane-per-replicate fill (halves of 33 .. 64 live replicates, full tiles)
    loops, worst = {}, 0
    for c in GROUP_A:
        counts, freq = cached_reference(orc, c)
        worst = max(worst, int(freq.max()))
        nt = counts.shape[1]
        full_tiles = nt if c["N"] % TILE == 0 else nt - 1
        hit = set()
        for h, lab in enumerate(c["halves"]):
            if lab in ("full", "dead lanes"):
                r0 = c["rep_begin"] + HALF * h
                for t in range(full_tiles):
                    n = counts[r0:min(r0 + HALF, c["nrep"]), t].astype(np.int64)
                    hit |= philox_loops(int(n.min()), int(n.max()))
        loops[c["id"]] = hit
    assert set().union(*loops.values()) == {"two chains", "one chain", "ragged"}
    assert loops["N3000-r100-nsamp5"] == {"ragged"}                   # nmin < 12: no call is complete for every lane
    assert loops["N5000-r330-top"] == {"two chains", "one chain", "ragged"}
    # some (replicate, tile) draws nothing: the one-sample last tile of N = 1025
    counts, _ = cached_reference(orc, by_id["N1025-r130"])
    assert (counts[:, 1] == 0).any() and (counts[:, 1] > 0).any()
    counts, _ = cached_reference(orc, by_id["N3000-r100-nsamp5"])
    assert (counts == 0).sum() > 0 and counts.max() <= 5
    # the densest case (16 draws per sample on average) is far inside a byte
    _, freq = cached_reference(orc, by_id["N2047-r8-dense"])
    assert worst == int(freq.max()) <= 255
    print(f"largest count of the case table: {worst}")
