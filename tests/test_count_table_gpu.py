"""The count-table generator (`txm_sampler_count_table`, thermoextrap_amd/csrc/txm_count_table.hip) held, byte for byte,
to the CPU statement of its table: `oracle/count_table_oracle.encode` on the frequency rows of the CPU restatement of the
sampler stream (oracle/philox_oracle.c).  Every call goes through the C ABI into a buffer pre-filled with 0xFF, so a byte
the kernel does not write is seen.  Nothing here has a tolerance except group D, which reuses tests/test_i8_gpu.py's.

* A: bytes against the oracle, on the case table that tests/test_count_table_cpu.py proves to reach every path of the
  kernel -- the fill widths on both sides of each boundary, dead lanes, dead half groups, full and slid partial tiles,
  the three Philox loops, slabs that start past replicate 0 and slabs that reach past nrep, the top of the stream range,
  nsamp != ndat.
* B: a run of several tiles per workgroup (launch_count_table's rule restated), against the device's own frequency rows.
* C: bits that must not move -- repeated calls, the buffer's previous content, slabs against the whole call and against
  a sampler of the slab's rows, the packed fill against the lane-per-replicate fill.
* D: the consumer at a small shape, every replicate against the long-double definition.
* E: refusals leave the buffer untouched.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import count_table_oracle as cto
from test_count_table_cpu import GROUP_A, SEED, cached_reference, half_labels, tile_kinds
from test_i8_gpu import TOL, data, truth_err

pytestmark = pytest.mark.gpu

TILE_BYTES = 131072
ERR_INVALID = -1     # include/txmom.h TXM_ERR_INVALID


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


@pytest.fixture(scope="module")
def L(txm):
    from thermoextrap_amd import _lib

    return _lib.load()


def call(L, eng, spec, counts, rep_begin, nreps, table):
    rc = L.txm_sampler_count_table(ct.byref(spec), eng._ptr(counts), rep_begin, nreps, eng._ptr(table), eng._stream())
    torch.cuda.synchronize()
    return rc


def make_table(L, eng, s, rep_begin, nreps, fill=0xFF):
    nb = L.txm_sampler_count_table_bytes(s.ndat, nreps)
    assert nb == cto.count_table_bytes(s.ndat, nreps) and nb > 0
    t = torch.full((nb,), fill, dtype=torch.uint8, device="cuda")
    rc = call(L, eng, s.spec, s.counts, rep_begin, nreps, t)
    assert rc == 0, (rc, L.txm_last_error())
    return t


def where(i, ntiles):
    """A byte offset in the header's coordinates, for the message of a failed comparison."""
    return dict(g=i // (TILE_BYTES * ntiles), t=(i // TILE_BYTES) % ntiles, s=(i // 4096) % 32, q=(i // 1024) % 4, L=(i // 16) % 64, b=i % 16)


def assert_same_bytes(got, want, ntiles, what):
    """torch.equal, with the first differing bytes named when it fails."""
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want).flatten()
    first = [(where(int(i), ntiles), int(got[i]), int(want[i])) for i in bad[:4]]
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} bytes differ; first (where, got, want): {first}")


def windows(table, ntiles, groups):
    """The table as [groups * 128 replicates][ntiles][1024 window positions] (a device restatement of `decode`'s
    permutation; the windows are not summed into rows, so this is a bijection of the bytes)."""
    a = table.view(groups, ntiles, 32, 4, 2, 32, 16)          # g t s q half n32 b
    return a.permute(0, 3, 5, 1, 2, 4, 6).reshape(groups * 128, ntiles, 1024)


# ---- A: bytes against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUP_A, ids=[c["id"] for c in GROUP_A])
def test_table_is_the_oracles_bytes(L, eng, orc, c):
    assert c["seed"] >> 32
    assert half_labels(c["nrep"], c["rep_begin"], c["nreps"]) == c["halves"]        # the paths the case is named for
    kinds, shift = tile_kinds(c["N"])
    counts, freq = cached_reference(orc, c)
    s = eng.DeviceSampler(c["seed"], c["nrep"], c["N"], nsamp=c["nsamp"], rep0=c["rep0"])
    assert np.array_equal(s.counts.cpu().numpy().view(np.uint32), counts)
    want = torch.from_numpy(cto.encode(freq, c["N"], c["nrep"], c["rep_begin"], c["nreps"]))
    got = make_table(L, eng, s, c["rep_begin"], c["nreps"]).cpu()
    print(f"\n{c['id']}: slab [{c['rep_begin']}, +{c['nreps']}) of {c['nrep']}, {got.numel()} bytes, halves {c['halves']}, tiles "
          f"{sorted(kinds)} shift {shift}, largest count {int(freq.max())}, bytes differing from the oracle: {int((got != want).sum())}")
    assert_same_bytes(got, want, s.ntiles, c["id"])


# ---- B: runs of several tiles per workgroup ----------------------------------------------------------------------------
def tiles_per_block(ntiles, n_groups, cus):
    """launch_count_table's rule."""
    tpb = 32
    while tpb > 1 and -(-ntiles // tpb) * 2 * n_groups < 4 * cus:
        tpb //= 2
    return tpb


def test_runs_of_several_tiles_per_workgroup(L, eng, orc):
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    n_groups = 8
    while True:
        ntiles = next(n for n in range(3, 1 << 20, 2) if tiles_per_block(n, n_groups, cus) >= 2)
        if n_groups * ntiles * TILE_BYTES <= 512 << 20:
            break
        n_groups += 8
    nrep = 1000 if n_groups == 8 else 128 * n_groups - 24
    N = 1024 * (ntiles - 1) + 300
    tpb = tiles_per_block(ntiles, n_groups, cus)
    assert tpb >= 2 and ntiles % tpb != 0 and -(-nrep // 128) == n_groups
    own = 1024 * (ntiles - 1) - (N - 1024)                     # window positions of the last tile that are its own samples
    assert own == 1024 - 300
    seed = SEED + 0xB00000000
    s = eng.DeviceSampler(seed, nrep, N)
    table = make_table(L, eng, s, 0, nrep)
    assert table.numel() == n_groups * ntiles * TILE_BYTES
    got = windows(table, ntiles, n_groups)
    wrong = 0
    for g in range(n_groups):
        live = min(128, nrep - 128 * g)
        f = s.rows(128 * g, 128 * g + live).freq()             # held to the CPU restatement by tests/test_kernels_gpu.py
        assert 0 <= int(f.min()) and int(f.max()) <= 255
        want = torch.zeros((128, ntiles, 1024), dtype=torch.uint8, device="cuda")
        want[:live, :ntiles - 1] = f[:, :1024 * (ntiles - 1)].reshape(live, ntiles - 1, 1024).to(torch.uint8)
        want[:live, ntiles - 1, own:] = f[:, 1024 * (ntiles - 1):].to(torch.uint8)
        bad = int((got[128 * g:128 * g + 128] != want).sum())
        wrong += bad
        assert bad == 0, (g, bad)
    # group 0's first rows against the CPU oracle as well
    rows = cto.decode(table[:ntiles * TILE_BYTES].cpu().numpy(), N, 128)[:16]
    assert np.array_equal(rows, orc.sampler_freq(seed, 16, N))
    print(f"\n{cus} CUs: {ntiles} tiles in runs of {tpb}, {n_groups} groups ({nrep} replicates), N = {N}, table {table.numel()} bytes: "
          f"bytes differing from the device's frequency rows {wrong}; group 0 rows 0-15 equal the CPU oracle")


# ---- C: bits that must not move ----------------------------------------------------------------------------------------
def test_same_bytes_whatever_was_there_and_however_the_slab_is_cut(L, eng):
    N, nrep, seed = 5000, 330, SEED + 0xC00000000
    s = eng.DeviceSampler(seed, nrep, N, rep0=77)
    whole = make_table(L, eng, s, 0, nrep)
    assert torch.equal(make_table(L, eng, s, 0, nrep), whole)                      # the same call twice
    assert torch.equal(make_table(L, eng, s, 0, nrep, fill=0x00), whole)           # nothing of the buffer's content survives
    k = nrep - 128
    assert half_labels(nrep, 128, k) == ("full", "full", "full", "pack 4")
    slab = make_table(L, eng, s, 128, k)
    assert torch.equal(slab, whole[s.ntiles * TILE_BYTES:])                        # groups 1 and onward of the whole call
    assert torch.equal(make_table(L, eng, s.rows(128, nrep), 0, k), slab)          # ... and the rows as a sampler of their own
    print(f"\nN = {N}, nrep = {nrep}: repeated call, 0x00 / 0xFF pre-fill, slab (128, {k}) and rows(128, {nrep}): same bytes")


def test_packed_fill_writes_the_bytes_of_the_lane_per_replicate_fill(L, eng):
    """Replicates 64..71 are the packed half group (8 lanes per replicate) of a 72-replicate call and 8 of the 64 lanes of
    a full half group in a 128-replicate call on the same seed."""
    N, seed = 2047, SEED + 0xC00000001
    assert half_labels(72, 0, 72) == ("full", "pack 8") and half_labels(128, 0, 128) == ("full", "full")
    a = windows(make_table(L, eng, eng.DeviceSampler(seed, 72, N), 0, 72), 2, 1)
    b = windows(make_table(L, eng, eng.DeviceSampler(seed, 128, N), 0, 128), 2, 1)
    assert torch.equal(a[:72], b[:72]) and int(a[64:72].sum()) == 8 * N
    assert not a[72:].any() and int(b[72:].sum()) == 56 * N
    print(f"\nN = {N}: replicates 64..71, pack 8 (nrep 72) and full (nrep 128): same bytes")


# ---- D: the consumer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrep,last", [(90, "pack 2"), (200, "pack 8"), (330, "pack 4")])
def test_table_fed_bootstrap_every_replicate_against_the_definition(eng, orc, nrep, last):
    N, C, order, seed = 5000, 32, 1, SEED + 0xD00000000
    assert [h for h in half_labels(nrep, 0, nrep) if h != "dead half"][-1] == last
    x, u = data(N, C, 17)
    w = 0.25 + torch.rand(N, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(19))
    s = eng.DeviceSampler(seed, nrep, N)
    got = eng.resample_vals(x, u, order, sampler=s, w=w, path="int8_table")
    assert eng.resample_info()["kernel"] == "int8_table"
    assert got.shape == (nrep, C, 2, order + 1)
    freq = torch.from_numpy(orc.sampler_freq(seed, nrep, N))
    e = truth_err(orc, got, x, u, order, freq, range(nrep), w=w)
    print(f"\nnrep = {nrep} (last live half group: {last}): worst of {nrep} replicates against the long-double definition {e:.3e} (limit {TOL:g})")
    assert e < TOL, e


# ---- E: refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffer_untouched(L, eng):
    from thermoextrap_amd._lib import SamplerSpec

    N, nrep = 2047, 130
    s = eng.DeviceSampler(SEED + 0xE00000000, nrep, N)
    buf = torch.full((L.txm_sampler_count_table_bytes(N, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    short = eng.DeviceSampler(SEED + 0xE00000000, nrep, 1024)
    spec1023 = SamplerSpec(seed=short.spec.seed, nrep=nrep, ndat=1023, nsamp=0, rep0=0)     # its one count column is a valid buffer
    for what, spec, counts, rb, nr, table in (
            ("rep_begin = 64", s.spec, s.counts, 64, 64, buf),
            ("rep_begin = 1", s.spec, s.counts, 1, 128, buf),
            ("rep_begin = 256 >= nrep", s.spec, s.counts, 256, 1, buf),
            ("rep_begin = 128 = nrep", s.rows(0, 128).spec, s.counts, 128, 1, buf),
            ("nreps = 0", s.spec, s.counts, 0, 0, buf),
            ("nreps = -1", s.spec, s.counts, 0, -1, buf),
            ("ndat = 1023", spec1023, short.counts, 0, nrep, buf),
            ("null table", s.spec, s.counts, 0, nrep, None)):
        rc = call(L, eng, spec, counts, rb, nr, table)
        assert rc == ERR_INVALID, (what, rc)
        assert bool((buf == 0xFF).all()), what
        print(f"\nrefused ({rc}): {what}: {L.txm_last_error().decode()}")
    for ndat, nr in ((1023, 130), (0, 1), (5000, 0), (5000, -3)):
        assert L.txm_sampler_count_table_bytes(ndat, nr) == 0
    assert call(L, eng, s.spec, s.counts, 128, 2, buf) == 0          # the buffer and the sampler were good all along
    assert not bool((buf[:2 * TILE_BYTES] == 0xFF).any()) and bool((buf[2 * TILE_BYTES:] == 0xFF).all())
