"""Synthetic code-block content for the HT block coder tests: magnitudes below 2^top, chosen to reach what breaks block coders.
Shared by the GPU tests of the int16 instances (test_gpu_ht_planes16.py) and the CPU pin of their reference (test_oracle_golden.py)."""
import numpy as np

# the four positions of a quad in the first / last quad row and column of a block: (last quad row?, last quad column?, dy, dx)
S_POSITIONS = [(qy, qx, dy, dx) for qy in (0, 1) for qx in (0, 1) for dy in (0, 1) for dx in (0, 1)]
MODES = [0, 1, 2, 3, 4, 5, "P"]
Q_KINDS = ["checker", "first_row", "not_first_row"]


def magnitudes(rng, bh, bw, top, mode):
    """(bh, bw) magnitudes < 2^top.  0 uniform; 1 shifted down at random; 2 sparse (93 % zeros) and large; 3 all zero; 4 all at
    2^top - 1 (0xFF-dense MagSgn: the stuffing paths); 5 wide and narrow quads side by side; "P": every sample one of 2^k - 1,
    2^k, 2^k + 1 for random k < top, clipped below 2^top -- where the exponent (the leading-bit count of 2 mag - 1) steps."""
    if mode == 0:
        return rng.integers(0, 1 << top, size=(bh, bw))
    if mode == 1:
        return rng.integers(0, 1 << top, size=(bh, bw)) >> rng.integers(0, top + 1, size=(bh, bw))
    if mode == 2:
        return np.where(rng.random((bh, bw)) < 0.93, 0, rng.integers(0, 1 << top, size=(bh, bw)))
    if mode == 3:
        return np.zeros((bh, bw), np.int64)
    if mode == 4:
        return np.full((bh, bw), (1 << top) - 1, np.int64)
    if mode == 5:
        wide = np.kron(rng.random(((bh + 1) // 2, (bw + 1) // 2)) < 0.3, np.ones((2, 2), bool))[:bh, :bw]
        return np.where(wide, rng.integers(1 << (top - 1), 1 << top, size=(bh, bw)), rng.integers(0, 16, size=(bh, bw)))
    if mode == "P":
        k = rng.integers(0, top, size=(bh, bw))
        return np.clip((1 << k) + rng.integers(-1, 2, size=(bh, bw)), 0, (1 << top) - 1)
    raise ValueError(mode)


def single_sample(bh, bw, position, mag):
    """all zero but one sample of magnitude `mag` at S_POSITIONS[position] (clipped into the block where it is ragged)"""
    qy, qx, dy, dx = S_POSITIONS[position % len(S_POSITIONS)]
    QH, QW = (bh + 1) // 2, (bw + 1) // 2
    y = min(2 * (QH - 1 if qy else 0) + dy, bh - 1)
    x = min(2 * (QW - 1 if qx else 0) + dx, bw - 1)
    m = np.zeros((bh, bw), np.int64)
    m[y, x] = mag
    return m


def quad_pattern(rng, bh, bw, top, kind):
    """significant quads (every sample in 1 .. 2^top - 1) in a checkerboard of quads / in the first quad row only / in every quad
    row but the first, the other quads empty: MEL runs of context-0 quads that end with the block, the first row's UVLC mode"""
    qy, qx = np.mgrid[0:(bh + 1) // 2, 0:(bw + 1) // 2]
    on = {"checker": (qy + qx) % 2 == 0, "first_row": qy == 0, "not_first_row": qy > 0}[kind]
    on = np.kron(on, np.ones((2, 2), bool))[:bh, :bw]
    return np.where(on, rng.integers(1, 1 << top, size=(bh, bw)), 0)


def signed(rng, mag):
    return mag * np.where(rng.random(mag.shape) < 0.5, -1, 1)
