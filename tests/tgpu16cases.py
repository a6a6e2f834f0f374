"""Layouts and the table checker of the 16-bit torch-GPU-order plans
(fa_plan_create_order_elem), shared by tests/test_tgpu16_cpu.py and
tests/test_gpu_tgpu16_kernel.py.  No GPU here: the tables come from the
library's host entry fa_plan_build_order_host_elem."""
import ctypes

import numpy as np

from feddct_amd import _lib
from feddct_amd.layout import BucketLayout

ELEMS = {"float16": _lib.FA_ELEM_F16, "bfloat16": _lib.FA_ELEM_BF16}
GAPS = _lib.FA_PLAN_GAPS_ARE_PADDING

# tile kinds (csrc/tiles.h)
K_SCALAR, K_SCALAR64, K_INNER, K_INNER64, K_V, K_W = 7, 8, 9, 10, 11, 12

KEY_SIZES = [1, 2, 3, 6, 8, 16, 36, 100, 128, 2047, 2048, 4097, 3 * 2048, 5 * 2048 + 100]
PLAN_NS = [2, 9, 17, 32, 64, 128, 256]


def manifest_layout(dtype, sizes=tuple(KEY_SIZES)):
    """The native 16-bit layout of one key per size plus an int64 0-dim key."""
    ent = [(f"t{j}", (m,) if m > 1 else (), dtype) for j, m in enumerate(sizes)]
    ent.insert(3, ("nbt", (), "int64"))
    return BucketLayout(ent, native16=True)


def raw_segments(n=2):
    """(segs [k, 2], bucket numel): for every residue r mod 8 a group of keys
    back to back whose first starts at r past an 8-element boundary (so the
    later ones start at every other residue too), small gaps between the
    groups, then three aligned keys back to back (one vector run) and a
    one-element key between two aligned ones (it breaks the run).  The small
    key has 9 elements, or 33 from N = 256 on, where torch's block is higher
    than 16 rows for every key below 32 elements (outside the restatement)."""
    small = 9 if n < 256 else 33
    segs, off = [], 0
    for r in range(8):
        off = (off + 7) // 8 * 8 + r
        for m in (2048 + 17, small, 1, 40 + r):
            segs.append((off, m))
            off += m
        off += 3
    off = (off + 7) // 8 * 8
    for m in (128, 256, 2048 * 2):
        segs.append((off, m))
        off += m
    off += 16                      # a gap a padded run may cross
    segs.append((off, 512))
    off += 512
    segs.append((off, 1))
    off += 8
    segs.append((off, 64))
    off += 64
    numel = (off + 7) // 8 * 8 + 64
    return np.array(segs, np.int64), numel


def config(n, m):
    """fa_torch_gpu_config's (inside, S) for a key of m elements."""
    st = ctypes.c_int(0)
    ok = _lib.lib.fa_torch_gpu_config(int(n), int(m), ctypes.byref(st))
    return bool(ok), st.value


def factor(n, m):
    """torch's float(num_outputs) / float(numel), in fp32."""
    return np.float32(m) / np.float32(n * m)


def check_table(segs32, numel32, segs64, numel64, n, flags, elem, tiles, fac, lo):
    """Every property a torch-GPU-order table must have, whatever cut it."""
    segs32 = np.asarray(segs32, np.int64).reshape(-1, 2)
    segs64 = np.asarray(segs64, np.int64).reshape(-1, 2)
    vec, wmax, vmax = (8, 2048, 2048) if elem != _lib.FA_ELEM_F32 else (4, 2048, 1024)
    key_of = {False: np.full(numel32, -1, np.int64), True: np.full(max(numel64, 1), -1, np.int64)}
    for is64, segs in ((False, segs32), (True, segs64)):
        for i, (o, m) in enumerate(segs):
            key_of[is64][o:o + m] = i
    cover = {False: np.zeros(numel32, np.int32), True: np.zeros(max(numel64, 1), np.int32)}
    assert len(tiles) == len(fac) == lo[5] and lo[0] == 0
    assert all(lo[g] <= lo[g + 1] for g in range(5)), lo
    for i, ((start, count, kind), f) in enumerate(zip(tiles, fac)):
        base, ls, vbit = kind & 0xFF, (kind >> 8) & 0xFF, (kind >> 16) & 1
        is64 = base in (K_SCALAR64, K_INNER64)
        inner = base in (K_INNER, K_INNER64)
        assert base in (K_SCALAR, K_SCALAR64, K_INNER, K_INNER64, K_V, K_W), kind
        assert count > 0 and start >= 0
        cover[is64][start:start + count] += 1
        if base in (K_V, K_W):
            assert start % vec == 0 and count % vec == 0, (start, count, kind)
            assert count <= (wmax if base == K_W else vmax), (count, kind)
            assert (ls <= 1) == (base == K_W), kind
        elif inner:
            assert count <= 4
        else:
            assert count <= 256
        keys = np.unique(key_of[is64][start:start + count])
        keys = keys[keys >= 0]
        assert keys.size >= 1
        for k in keys:
            m = int((segs64 if is64 else segs32)[k, 1])
            ok, s = config(n, m)
            assert ok and (1 << ls) == s, (kind, m, s)
            assert inner == (m == 1) and vbit == (1 if inner and n >= 128 else 0), (kind, m)
            assert np.float32(f).tobytes() == factor(n, m).tobytes(), (f, n, m)
        # its launch group: its own row split (inner tiles with S = 1), or a
        # rider in the S = 2 launch
        g = next(g for g in range(5) if lo[g] <= i < lo[g + 1])
        own = 0 if inner else ls
        assert g == own or (g == 1 and own in (0, 2)), (g, kind)
    for is64 in (False, True):
        inside = key_of[is64] >= 0
        assert (cover[is64][inside] == 1).all(), "a segment element outside exactly one tile"
        if is64 or not (flags & GAPS):
            assert (cover[is64][~inside] == 0).all(), "a tile crosses a gap that is not padding"
        else:
            assert (cover[is64][~inside] <= 1).all()
