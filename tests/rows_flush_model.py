"""The 1-row-slice encoder's batched flush policy (csrc/slice_kernels.hip, "Staging area") as a model on the oracle's byte counts, for
test_rows_encoder_flush_model.py (CPU) and test_gpu_rows_encoder_issue.py.

A lane stages its output bytes in kStageBytes of LDS.  Once per sample, in front of its coding, the wavefront asks whether ANY of its
lanes holds at least kFlushAt bytes; if so, every lane that holds a whole 16-byte unit stores one.  The first renormalisation of a
slice emits a dummy byte at position -1, which is the LAST byte of the neighbouring lane's area: that byte must never hold output, so
the fill may reach kStageBytes - 1 and no more.  finish() first stores a unit if there is one, then adds its two bytes."""
import os
import re

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llcomp_amd", "csrc", "slice_kernels.hip")


def constants():
    """kStageBytes, kSampleBytesMax, kFlushAt as the kernel source has them"""
    text = open(_SRC).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kStageBytes", "kSampleBytesMax", "kFlushAt"))


def renorms_per_sample(orc, row):
    """row: int16 (w,) plane values of a one-row slice -> int array (w,): renormalisations (bytes, the dummy one included) per sample.
    A stream of k samples is as long as the renormalisations of those samples plus finish()'s two, less the dummy byte."""
    w = len(row)
    total = np.array([len(orc.encode_samples(row[:k].reshape(1, k, 1))) - 1 for k in range(1, w + 1)], dtype=np.int64)
    return np.diff(np.concatenate([[0], total]))


class Wave:
    """the staging areas of the lanes of one wavefront under the batched policy.  `alone`: every lane is treated as if no other lane
    ever reached the threshold (the fewest flushes a lane can see); otherwise the lanes of the wavefront trigger each other."""

    def __init__(self, counts, alone=False):
        self.stage, self.most, self.at = constants()
        self.counts = [np.asarray(c, dtype=np.int64) for c in counts]
        self.alone = alone
        self.fill = np.full(len(counts), -1, dtype=np.int64)  # position -1: the dummy byte
        self.peak = 0
        self.events = self.stores = 0
        self.unit_at_finish = []

    def run(self):
        for s in range(max(len(c) for c in self.counts)):
            live = np.array([s < len(c) for c in self.counts])
            ready = live & (self.fill >= self.at)
            if ready.any():
                go = ready if self.alone else live & (self.fill >= 16)
                self.fill[go] -= 16
                self.events += 1
                self.stores += int(go.sum())
            assert (self.fill[live] < self.at).all(), "one unit per lane and flush event was not enough"
            for i, c in enumerate(self.counts):
                if s < len(c):
                    assert c[s] <= self.most, ("a sample added more bytes than kSampleBytesMax", int(c[s]))
                    self.fill[i] += c[s]
                    if s == len(c) - 1:  # finish(): a unit first if there is one, then two more bytes
                        self.peak = max(self.peak, int(self.fill[i]))
                        self.unit_at_finish.append(bool(self.fill[i] >= 16))
                        self.fill[i] = self.fill[i] % 16 + 2 if self.fill[i] >= 0 else 1
            self.peak = max(self.peak, int(self.fill.max()))
            assert self.peak <= self.stage - 1, ("output reached the byte that takes the neighbour's dummy byte", self.peak)
        return self
