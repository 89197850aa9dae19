"""The one fixed shape of the device's two-level sums (fast_limo_amd/csrc/hip/flimo_sums.h), restated in numpy.

Slots are cut into segments of SEG; in a segment thread t of RED adds the terms of slots t, t + RED, .. in ascending order onto an
accumulator that starts at +0.0, inside a slot the slot's terms in ascending order; an xor butterfly over the 64 lanes of each of
the four waves; ((wave 0 + wave 1) + (wave 2 + wave 3)); the segments' partials are added in ascending order onto +0.0.  A slot
past the end adds nothing on the device and +0.0 here: an accumulator that starts at +0.0 is never -0.0, so the bits are the same.
flimo_scan_linearize, flimo_scan_ndt and flimo_map_outliers are pinned to this function bit for bit."""
import numpy as np

SEG, RED = 4096, 256


def shape_sums(T):
    """T [n, terms_per_slot, N] float64 -> the N sums [N]."""
    T = np.asarray(T, np.float64)
    n, per, N = T.shape
    total = np.zeros(N)
    for s0 in range(0, n, SEG):
        blk = np.zeros((SEG, per, N))
        m = min(SEG, n - s0)
        blk[:m] = T[s0:s0 + m]
        seq = blk.reshape(SEG // RED, RED, per, N).transpose(1, 0, 2, 3).reshape(RED, -1, N)      # thread t: slots t, t + 256, ..
        acc = np.zeros((RED, N))
        for j in range(seq.shape[1]):
            acc = acc + seq[:, j]
        lanes = acc.reshape(4, 64, N)
        idx = np.arange(64)
        o = 1
        while o < 64:
            lanes = lanes + lanes[:, idx ^ o]
            o <<= 1
        wv = lanes[:, 0]
        total = total + ((wv[0] + wv[1]) + (wv[2] + wv[3]))
    return total
