"""Coefficient planes of the tests' choosing for the rate-targeted encodes' kernels (tests/test_gpu_rate.py: the block coder's drop
instances; tests/test_gpu_rate_tables.py: the statistics): one component, 2 levels, magnitudes chosen block by block."""
import ctypes as C

import numpy as np

import grok_amd as G
import gpuutil as U
import ht_content as HC
import oracle as O

FORMS = {"int32 reversible": (12, False, False), "int32 irreversible": (12, True, False), "int16": (8, False, True)}     # prec, 9/7, int16 planes
GEOMS = {"cblk 64": (128, 128, (6, 6)), "cblk 32": (128, 128, (5, 5)), "cblk 4": (128, 128, (2, 2)), "ragged 77x53": (77, 53, (5, 5))}
# ... and one more for the statistics alone: a block as wide as a wave beside a ragged one
STATS_GEOMS = dict(GEOMS, **{"200x70 cblk 64": (200, 70, (6, 6))})


def planes_case(form, geom, seed, mode_of=None, signmag=True):
    """one component, 2 levels: -> (params, blocks, the device planes, planes16, [sign-magnitude words of every block as the d = 0
    coder sees them], the host planes (1, H, W): integers, or float32 for 9/7).
    form: a name of FORMS or (prec, 9/7, int16 planes); geom: a name of STATS_GEOMS.  mode_of(i): block i's content -- a mode of
    ht_content.magnitudes, ("below", m): uniform below m, or a callable (rng, bh, bw, block) -> magnitudes.  signmag = False: no
    sign-magnitude words (content beyond the quantiser's clamp has none the oracle would agree with)."""
    prec, irrev, h16 = FORMS[form] if isinstance(form, str) else form
    W, H, cblk = STATS_GEOMS[geom]
    p = G.TileParams.make(W, H, 1, prec, 2, irreversible=irrev, mct=False, cblk=cblk)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(seed)
    modes = [0, 1, 2, 5, "P", 4]
    mags = np.zeros((H, W), np.int64)
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        mode = mode_of(i) if mode_of else modes[i % len(modes)]
        if callable(mode):
            m = mode(rng, bh, bw, b)
        elif isinstance(mode, tuple):
            m = rng.integers(0, mode[1], (bh, bw))
        else:
            m = HC.magnitudes(rng, bh, bw, b.kmax, mode)
        mags[b.py:b.py + bh, b.px:b.px + bw] = m
    sgn = np.where(rng.random((H, W)) < 0.5, -1, 1)
    sms = []
    if irrev:
        planes = np.zeros((1, H, W), np.float32)
        for b in blocks:
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            sl = (slice(b.py, b.py + bh), slice(b.px, b.px + bw))
            planes[0][sl] = (sgn[sl] * (mags[sl] + np.where(mags[sl] > 0, 0.37, 0.0)) * float(b.stepsize)).astype(np.float32)
            if not signmag:
                continue
            sub = np.ascontiguousarray(planes[0][sl])
            sm = np.zeros((bh, bw), np.uint32)
            O.lib().orc_ht_signmag_irrev(sub.ctypes.data, bw, bw, bh, b.kmax, C.c_float(np.float32(1.0) / np.float32(b.stepsize)), sm.ctypes.data)
            assert np.array_equal((sm & 0x7FFFFFFF) >> (30 - b.kmax), mags[sl])
            sms.append(sm)
        dev = U.upload_planes(planes.view(np.int32), p)
    else:
        planes = (sgn * mags)[None]
        for b in blocks:
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            if signmag:
                sms.append(O.signmag(planes[0, b.py:b.py + bh, b.px:b.px + bw], b.kmax))
        dev = U.upload_planes16(planes, p) if h16 else U.upload_planes(planes.astype(np.int32), p)
    return p, blocks, dev, h16, sms, planes
