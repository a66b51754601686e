"""The host code that fills a tier-B launch's constants (launch_philox's fill_frame_geometry /
fill_batch_geometry, rt_render.hip) against an independent decomposition in Python integers: the divisors
(Granlund-Montgomery constants) and the geometry must reproduce work_item / work_unit for a small frame —
every shard, the last (tail) shard with its padding tiles included, chunk batches, and a sample-granular
tail. rt_internal_work_units evaluates the device's own work_unit code on the host; no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import rtamd

K_TAIL_SLOT = 1 << 40


def _units(p, chunk_first, n_chunks, tail_items):
    fn = rtamd.lib().rt_internal_work_units
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    totals = np.zeros(5, dtype=np.int64)
    assert fn(C.addressof(p), chunk_first, n_chunks, tail_items, 0, 0, None, None, totals.ctypes.data) == 0
    n = int(totals[0])
    out5 = np.zeros((n, 5), dtype=np.int32)
    slot = np.zeros(n, dtype=np.int64)
    assert fn(C.addressof(p), chunk_first, n_chunks, tail_items, 0, n, out5.ctypes.data, slot.ctypes.data,
              totals.ctypes.data) == 0
    return totals, out5, slot


def _expected_item(wi, p, tile, slab, chunk, chunk_first, n_chunks):
    """work_item by definition: items run tile by tile, chunk by chunk inside a tile, 8x8 blocks inside a tile;
    a shard owns the tiles rank, rank + shards, ..."""
    W, H, spp = p.width, p.height, p.spp
    shards = max(1, p.shard_count)
    tiles_x, tiles_y = -(-W // tile), -(-H // tile)
    tp = tile * tile
    lt, rem = divmod(wi, tp * n_chunks)
    k, within = divmod(rem, tp)
    idx = lt * tp + within
    gt = p.shard_rank + lt * shards
    if gt >= tiles_x * tiles_y:
        return None
    ty, tx = divmod(gt, tiles_x)
    blk, lane = divmod(within, 64)
    by, bx = divmod(blk, tile // 8)
    px, row = tx * tile + bx * 8 + (lane & 7), ty * tile + by * 8 + (lane >> 3)
    if px >= W or row >= H:
        return None
    s0 = (chunk_first + k) * chunk
    s1 = min(spp, s0 + chunk)
    if s0 >= s1:
        return None
    return px, row, s0, s1, k * slab + idx


@pytest.mark.parametrize("w,h,spp,tile,shards,chunk,span,tail_items", [
    (20, 13, 11, 8, 1, 0, None, 0),       # ragged edges; the frame's own chunk size (1 at this size)
    (20, 13, 11, 8, 4, 0, None, 0),       # 6 tiles on 4 shards: shards 2 and 3 own one tile and one padding tile
    (37, 21, 11, 16, 5, 3, None, 0),      # chunks of 3 samples (the last one short), tile 16, 6 tiles on 5 shards
    (37, 21, 23, 16, 5, 3, (2, 4), 0),    # a chunk batch in the middle of the frame
    (24, 24, 11, 8, 2, 3, None, 100),     # a sample-granular tail
    (24, 24, 11, 8, 2, 3, (2, 2), 10 ** 9),  # the frame's last (short) chunk in a launch that is all tail
])
def test_work_units_match_the_definition(monkeypatch, w, h, spp, tile, shards, chunk, span, tail_items):
    if chunk:  # (small frames have 1-sample chunks: RTAMD_CHUNK sets the launch's chunk size)
        monkeypatch.setenv("RTAMD_CHUNK", str(chunk))
        chunks_total = -(-spp // chunk)
    else:
        monkeypatch.delenv("RTAMD_CHUNK", raising=False)
        chunk, chunks_total = rtamd.frame_chunking(w * h, spp)
    first, count = span if span else (0, chunks_total)
    assert first + count <= chunks_total
    covered = {}
    for rank in range(shards):
        p = rtamd.make_params(w, h, spp, 8, tile=tile, shard_rank=rank, shard_count=shards)
        _, _, slab = rtamd.shard_geometry(p)
        totals, out5, slot = _units(p, first, count, tail_items)
        work_total, items_total, tail_start, slab_c, chunk_c = (int(x) for x in totals)
        assert (slab_c, chunk_c) == (slab, chunk)
        assert items_total == slab * count
        tail = min(items_total, tail_items)
        assert tail_start == items_total - tail and work_total == items_total + tail * (chunk - 1)
        for wi in range(work_total):
            if wi < tail_start:
                exp = _expected_item(wi, p, tile, slab, chunk, first, count)
            else:  # one sample of a tail work-item per unit
                q, k = divmod(wi - tail_start, chunk)
                exp = _expected_item(tail_start + q, p, tile, slab, chunk, first, count)
                if exp is not None:
                    px, row, s0, s1, _ = exp
                    exp = (px, row, s0 + k, s0 + k + 1, K_TAIL_SLOT + wi - tail_start) if s0 + k < s1 else None
            ok, px, row, s0, s1 = (int(x) for x in out5[wi])
            if exp is None:
                assert not ok, (rank, wi)
                continue
            assert ok and (px, row, s0, s1, int(slot[wi])) == exp, (rank, wi, out5[wi], slot[wi], exp)
            for s in range(s0, s1):
                assert (px, row, s) not in covered, (rank, wi, px, row, s)
                covered[(px, row, s)] = rank
    # every sample of the span, of every image pixel, exactly once over the shards
    s_lo, s_hi = first * chunk, min(spp, (first + count) * chunk)
    assert len(covered) == w * h * (s_hi - s_lo)
    assert all(0 <= px < w and 0 <= row < h and s_lo <= s < s_hi for px, row, s in covered)
