"""Guard-banded buffers for the workspace / output contract tests (test_workspace_contract_gpu.py).

``Banded(nbytes, fill)`` is ONE ``torch.uint8`` allocation laid out as ``[BAND | payload | BAND]``: the payload is
256-byte aligned and exactly ``nbytes`` long, both bands hold ``0xA5`` and ``check()`` says whether they still do.  A
kernel that writes before or behind the memory it was promised lands in a band; a kernel that reads scratch it never
wrote reads the payload's fill:

  "zero"   all bytes 0
  "nan"    the 8-byte pattern 0x7FF8000000000000 repeated: a stale double is NaN, a stale 32-bit word is 0 or 0x7FF80000
  "value"  for output arrays: float64 NaN (``dtype`` float64) or all bits set, the integer -1 (integer ``dtype``)

``unwritten()`` counts the payload elements that still hold the "value" paint; ``holds_fill()`` says whether the whole
payload is still the fill it was given.  No test writes into a band on purpose.
"""

from __future__ import annotations

import numpy as np
import torch

BAND = 65536
BAND_BYTE = 0xA5
ALIGN = 256
NAN_BITS = 0x7FF8000000000000
_NAN_BYTES = np.frombuffer(np.uint64(NAN_BITS).tobytes(), dtype=np.uint8)   # little endian: 00 00 00 00 00 00 F8 7F


class Banded:
    def __init__(self, nbytes: int, fill: str = "nan", dtype=torch.float64, device="cuda"):
        if fill not in ("zero", "nan", "value"):
            raise ValueError(f"fill must be 'zero', 'nan' or 'value', got {fill!r}")
        self.nbytes = int(nbytes)
        if self.nbytes < 0:
            raise ValueError("nbytes must be >= 0")
        self.fill, self.dtype = fill, dtype
        self.raw = torch.empty(BAND + self.nbytes + BAND + ALIGN, dtype=torch.uint8, device=device)
        # the payload starts at the first 256-byte boundary at least BAND bytes into the allocation
        self.offset = BAND + (-(self.raw.data_ptr() + BAND)) % ALIGN
        self.front = self.raw[self.offset - BAND:self.offset]
        self.payload = self.raw[self.offset:self.offset + self.nbytes]
        self.back = self.raw[self.offset + self.nbytes:self.offset + self.nbytes + BAND]
        self.front.fill_(BAND_BYTE)
        self.back.fill_(BAND_BYTE)
        self.paint()

    def _pattern(self) -> torch.Tensor:
        if self.fill == "zero":
            return torch.zeros(self.nbytes, dtype=torch.uint8)
        if self.fill == "nan" or (self.fill == "value" and self.dtype.is_floating_point):
            if self.fill == "value" and self.dtype != torch.float64:
                raise ValueError("float outputs are float64")
            reps = -(-self.nbytes // 8)
            return torch.from_numpy(np.tile(_NAN_BYTES, reps)[:self.nbytes].copy())
        return torch.full((self.nbytes,), 0xFF, dtype=torch.uint8)

    def paint(self) -> None:
        """(Re)fill the payload."""
        if self.nbytes:
            self.payload.copy_(self._pattern().to(self.raw.device))

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + self.offset

    def view(self, dtype=None) -> torch.Tensor:
        """The payload as a 1-D tensor of ``dtype`` (default: the buffer's own)."""
        dtype = self.dtype if dtype is None else dtype
        return self.payload.view(dtype)

    def check(self) -> bool:
        """Both bands intact."""
        return bool((self.front == BAND_BYTE).all()) and bool((self.back == BAND_BYTE).all())

    def holds_fill(self) -> bool:
        """The whole payload still holds the fill (nothing wrote into it)."""
        return self.nbytes == 0 or bool((self.payload.cpu() == self._pattern()).all())

    def painted(self) -> torch.Tensor:
        """Per element of a "value" buffer: does it still hold the paint (bool, 1-D)."""
        if self.fill != "value":
            raise ValueError("painted() is for 'value' buffers")
        if self.dtype.is_floating_point:
            return self.payload.view(torch.int64) == NAN_BITS
        size = torch.empty((), dtype=self.dtype).element_size()
        return (self.payload.view(-1, size) == 0xFF).all(dim=1)

    def unwritten(self) -> int:
        """Elements of a "value" buffer that still hold the paint."""
        return int(self.painted().sum()) if self.nbytes else 0
