"""
oracle/count_table_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

CPU statement (pure numpy) of the u8 count table that ``txm_sampler_count_table`` writes, from the index formula in
``thermoextrap_amd/csrc/txm_i8g.h``:

    table[((g * ntiles + t) * 32 + s) * 4096 + q * 1024 + L * 16 + b]
        = draws of sample  tile_base(t) + 32 s + 16 (L >> 5) + b
          in replicate     128 g + 32 q + (L & 31)              of the slab,

``tile_base(t) = min(1024 t, N - 1024)``: the last tile slides its window back over samples that belong to the tile
before it; those foreign samples count 0 there (every sample is counted in exactly one tile).  Replicates at or past
``nrep`` count 0.  The slab is ``ceil(nreps / 128)`` groups of 128 replicates that start at call replicate
``rep_begin``.

``encode`` writes the table of a slab from the call's frequency rows, ``decode`` reads a table back into rows.  Both
know nothing about how the counts were drawn: the rows come from ``oracle.sampler_freq`` (oracle/philox_oracle.c) in
the tests, so that table = encode(CPU restatement of the stream) is a statement about every byte.
"""

from __future__ import annotations

import numpy as np

TILE = 1024        # samples per sampler tile (SM_T)
GROUP = 128        # replicates per group (G_REPS)
KSTEP = 32         # samples per k-step
TILE_BYTES = TILE * GROUP


def ntiles_of(N: int) -> int:
    return (N + TILE - 1) // TILE


def tile_base(t: int, N: int) -> int:
    return min(TILE * t, N - TILE)


def count_table_bytes(N: int, nreps: int) -> int:
    """txm_sampler_count_table_bytes: 0 for a series shorter than one tile or an empty slab."""
    if N < TILE or nreps < 1:
        return 0
    return ((nreps + GROUP - 1) // GROUP) * ntiles_of(N) * TILE_BYTES


def encode(freq, N: int, nrep: int, rep_begin: int, nreps: int) -> np.ndarray:
    """The table of the slab (rep_begin, nreps) of a call whose frequency rows are ``freq`` [nrep][N]: uint8[count_table_bytes]."""
    freq = np.asarray(freq)
    if freq.shape != (nrep, N):
        raise ValueError(f"freq has shape {freq.shape}, the call has {(nrep, N)}")
    if N < TILE or nreps < 1 or rep_begin < 0 or rep_begin % GROUP or rep_begin >= nrep:
        raise ValueError("count table: needs N >= 1024, nreps >= 1 and a slab that starts at a multiple of 128 inside the call")
    nt, G = ntiles_of(N), (nreps + GROUP - 1) // GROUP
    live = min(nrep - rep_begin, G * GROUP)          # slab rows that are replicates of the call
    rows = freq[rep_begin:rep_begin + live]
    if rows.min() < 0 or rows.max() > 255:
        raise ValueError(f"count table: counts {rows.min()} .. {rows.max()} do not fit a byte")
    # win[slab replicate][tile][position in the tile's window]
    win = np.zeros((G * GROUP, nt, TILE), dtype=np.uint8)
    for t in range(nt):
        b0 = tile_base(t, N)
        own = TILE * t - b0                          # window positions before this are the previous tile's samples
        win[:live, t, own:] = rows[:, b0 + own:b0 + TILE]
    # slab replicate = 128 g + 32 q + n32; window position = 32 s + 16 half + b; L = 32 half + n32
    a = win.reshape(G, 4, 32, nt, 32, 2, 16)         # g q n32 t s half b
    return np.ascontiguousarray(a.transpose(0, 3, 4, 1, 5, 2, 6)).reshape(-1)   # g t s q half n32 b


def decode(table, N: int, nreps: int) -> np.ndarray:
    """table -> int64 [ceil(nreps/128)*128][N] counts, undoing the operand order and the slid last tile."""
    nt, G = ntiles_of(N), (nreps + GROUP - 1) // GROUP
    a = np.asarray(table, dtype=np.uint8).reshape(G, nt, 32, 4, 2, 32, 16)       # g t s q half n32 b
    a = a.transpose(0, 3, 5, 1, 2, 4, 6).reshape(G * GROUP, nt, TILE)            # replicate, tile, position in the window
    out = np.zeros((G * GROUP, N), dtype=np.int64)
    for t in range(nt):
        b0 = tile_base(t, N)
        out[:, b0:b0 + TILE] += a[:, t]
    return out
