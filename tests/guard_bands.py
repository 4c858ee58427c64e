"""Guard bands around the tensors a kernel reads and writes (tests/test_hip_attention_edges.py, tests/test_hip_gemm_edges.py; on the CPU:
tests/test_gemm_probes_host.py).

`Banded` puts a view in the middle of a larger buffer. Inputs: everything outside the view is NaN, so a read past the view that feeds
a sum or a 0 * x product shows in the result. Outputs: the whole buffer holds a sentinel bit pattern (a finite, huge number in every dtype,
so an element the kernel leaves unwritten misses the reference), and bands_intact() finds a store outside the view. A contiguous view of
any rank sits between two bands; a two-dimensional view can also be a column block of wider rows (leading dimension `ld`, column offset
`col0`) with rows `row_step` apart and `pad_rows` whole rows behind the last one: then the pad columns between the view's columns and `ld`,
the rows between two rows of the view and the rows behind it belong to the bands.

The default sentinel is a value a kernel can store by chance where the range of the results is wide (0x5A5A is 203.25 in fp16): an output
can ask for one of NAN_SENTINEL instead, a NaN with a payload that no arithmetic produces (`sentinel=NAN_SENTINEL[dtype]`)."""
import math

import torch

BAND = 16384            # elements in front of and behind every placement: a multiple of 64, so a view keeps its 16-byte alignment
SENTINEL = {1: (torch.uint8, 0x5A), 2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5A5A5A), 8: (torch.int64, 0x5A5A5A5A5A5A5A5A)}
NAN_SENTINEL = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FDA5A5A}


class Banded:
    def __init__(self, shape, dtype, src=None, *, ld=None, col0=0, row_step=1, pad_rows=0, device="cuda", sentinel=None):
        shape = tuple(shape)
        if ld is None and col0 == 0 and row_step == 1 and pad_rows == 0:
            rows, cols = 1, math.prod(shape)      # contiguous, any rank
            ld, strides = cols, None
        else:
            rows, cols = shape
            ld = cols if ld is None else ld
            assert col0 >= 0 and col0 + cols <= ld and row_step >= 1
            strides = (row_step * ld, 1)
        self.rows, self.cols, self.ld, self.col0, self.row_step = rows, cols, ld, col0, row_step
        self.nrow = (rows - 1) * row_step + 1 + pad_rows            # rows of length ld the placement covers
        self.buf = torch.empty(2 * BAND + self.nrow * ld, device=device, dtype=dtype)
        self.itype, self.sent = SENTINEL[self.buf.element_size()]
        if sentinel is not None:
            self.sent = sentinel
        self.is_input = src is not None
        first = BAND + col0
        self.view = (self.buf[first:first + cols].view(shape) if strides is None
                     else self.buf.as_strided((rows, cols), strides, first))
        if self.is_input:
            if dtype.is_floating_point:
                self.buf.fill_(float("nan"))
            else:
                self.buf.view(self.itype).fill_(self.sent)
            self.view.copy_(src)
            self.before = self.buf.view(self.itype).clone()
        else:
            self.buf.view(self.itype).fill_(self.sent)
        assert self.view.data_ptr() % 16 == 0

    def _view_of(self, flat):
        """The positions of the view inside a flat tensor laid out like self.buf."""
        return flat.as_strided((self.rows, self.cols), (self.row_step * self.ld, 1), BAND + self.col0)

    def bands_intact(self):
        """Inputs: not one bit of the buffer changed (the bands and the view). Outputs: every element outside the view still holds the
        sentinel — the bands in front and behind, the pad columns, the rows between and behind the view's rows."""
        bits = self.buf.view(self.itype)
        if self.is_input:
            return torch.equal(bits, self.before)
        outside = bits.clone()
        self._view_of(outside).fill_(self.sent)
        return bool((outside == self.sent).all())

    def outside_intact(self):
        """A tensor a kernel reads AND writes (a gradient view it accumulates into), built like an input: nothing outside the view changed."""
        now, then = self.buf.view(self.itype).clone(), self.before.clone()
        self._view_of(now).fill_(0)
        self._view_of(then).fill_(0)
        return torch.equal(now, then)

    def unwritten(self):
        """Output: how many elements of the view still hold the sentinel."""
        return int((self._view_of(self.buf.view(self.itype)) == self.sent).sum())


def ptr(b):
    return None if b is None else b.view.data_ptr()
