"""GPU: the stager's zero-copy source path on a pinned staging chunk the host rewrites (stager.cpp launch_window:
pinned, mapped batch buffers and a window that fits one chunk -> the kernels read the chunk over PCIe with ordinary
loads, no H2D).  Six windows whose records have the same sizes -- so record i lies at the same chunk offset every
time -- and different pixels; every record of every window must equal the oracle bit for bit, and every launch
must report (aeon_hip_stager_last_launch) the path the test is about.  A stale cache line from the window before
shows as a mismatch.  A window of two chunks takes the H2D path and exercises the (chunk << 48) | offset rebasing.
"""
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests import helpers as H
from tests.buffers import Buffer

pytestmark = pytest.mark.gpu

SIZES = [(96, 64), (101, 67), (107, 70), (113, 71), (118, 73), (123, 75), (128, 76), (131, 77)]  # (w, h) of record i
BATCH, NBATCHES, NWIN = 4, 2, 6
MAXPIX = 131 * 77


def _pad16(n):
    return (n + 15) // 16 * 16


def _identity(w, h):
    return A.aug_params(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=w, out_h=h)


def _crop(i, w, h):
    return A.aug_params(crop_x=5 + i, crop_y=3 + i, crop_w=w - 11 - i, crop_h=h - 12 - i, out_w=32, out_h=24, flip=1)


class Lane:
    """One stager and what it is fed: per record i its source (from the window's image or mask) and params."""

    def __init__(self, ctx, name, out, mask, params):
        self.name, self.out, self.mask, self.params = name, out, mask, params
        self.stager = A.Stager(ctx, out, BATCH, A.STAGER_MASK if mask else A.STAGER_IMAGE)
        self.infos = []  # last_launch after each window's launch

    def nbytes(self, i):
        p = self.params[i]
        return p.out_w * p.out_h * self.out.channels * np.dtype(A.NP_DTYPE[self.out.dtype]).itemsize


def _lanes(ctx):
    ident = A.out_desc(channels=3, channel_major=False, bgr_to_rgb=False, dtype="uint8", item_stride=_pad16(MAXPIX * 3))
    small = A.out_desc(channels=3, channel_major=True, bgr_to_rgb=True, dtype="float32", mean=C.MEAN, stddev=C.STDDEV,
                       item_stride=3 * 24 * 32 * 4)
    masks = A.out_desc(channels=1, dtype="uint8", item_stride=_pad16(MAXPIX))
    return [Lane(ctx, "identity", ident, False, [_identity(w, h) for w, h in SIZES]),
            Lane(ctx, "crop", small, False, [_crop(i, w, h) for i, (w, h) in enumerate(SIZES)]),
            Lane(ctx, "mask", masks, True, [_crop(i, w, h) if i % 2 else _identity(w, h) for i, (w, h) in enumerate(SIZES)])]


def _window(win):
    """The window's records: (image, mask) of SIZES[i], pixels of their own in every window."""
    return [(A.synthetic_image(1000 * win + i, w, h, 3), A.synthetic_image(500000 + 1000 * win + i, w, h, 1))
            for i, (w, h) in enumerate(SIZES)]


def _stage(lanes, container, records):
    def one(i):
        for ln in lanes:
            ln.stager.stage(container[ln.name][i // BATCH].ptr, i % BATCH, records[i][1 if ln.mask else 0], ln.params[i])
    with ThreadPoolExecutor(max_workers=4) as pool:
        list(pool.map(one, range(len(records))))


def _check(lanes, copies, records, win):
    for ln in lanes:
        ref = H.oracle_records([r[1 if ln.mask else 0] for r in records], ln.params, ln.out, mask=ln.mask)
        for i, want in enumerate(ref):
            item = copies[(ln.name, i // BATCH)][(i % BATCH) * ln.out.item_stride:][:ln.nbytes(i)]
            got = item.view(A.NP_DTYPE[ln.out.dtype])
            assert got.size == want.size and np.array_equal(got, want.reshape(-1)), (win, ln.name, i)
    ident = copies[("identity", 0)][:SIZES[0][0] * SIZES[0][1] * 3]
    assert np.array_equal(ident, records[0][0].reshape(-1))  # (identity: every source byte is in the output)


@pytest.mark.parametrize("mode", ["flush", "overlap"])
def test_zero_copy_chunk_reuse(mode):
    ctx = A.Context(0)
    lanes = _lanes(ctx)
    ncont = 1 if mode == "flush" else 2
    containers = [{ln.name: [Buffer(BATCH * ln.out.item_stride, "pinned") for _ in range(NBATCHES)] for ln in lanes}
                  for _ in range(ncont)]
    windows = [_window(w) for w in range(NWIN)]
    try:
        if mode == "flush":  # one window object per stager: its chunk is rewritten every window
            for win, records in enumerate(windows):
                _stage(lanes, containers[0], records)
                for ln in lanes:
                    for b in range(NBATCHES):
                        ln.stager.flush(containers[0][ln.name][b].ptr)
                    ln.infos.append(ln.stager.last_launch())
                copies = {(ln.name, b): containers[0][ln.name][b].bytes() for ln in lanes for b in range(NBATCHES)}
                _check(lanes, copies, records, win)
        else:  # two containers: a chunk is rewritten every other window, while the other window's kernels may run
            free_q, full_q, errors = queue.Queue(), queue.Queue(), []
            for c in range(2):
                free_q.put(c)

            def decode_stage():
                try:
                    for win, records in enumerate(windows):
                        c = free_q.get(timeout=60)
                        _stage(lanes, containers[c], records)
                        for b in range(NBATCHES):  # post_process per batch: launch only
                            for ln in lanes:
                                ln.stager.launch(containers[c][ln.name][b].ptr)
                        for ln in lanes:
                            ln.infos.append(ln.stager.last_launch())
                        full_q.put((win, c))
                except Exception as e:  # surfaced below
                    errors.append(e)
                    full_q.put(None)

            th = threading.Thread(target=decode_stage)
            th.start()
            try:
                for _ in range(NWIN):  # the consumer
                    item = full_q.get(timeout=60)
                    assert item is not None, errors
                    win, c = item
                    copies = {}
                    for b in range(NBATCHES):
                        for ln in lanes:
                            A.Stager.wait_buffer(containers[c][ln.name][b].ptr)
                            copies[(ln.name, b)] = containers[c][ln.name][b].bytes()
                    free_q.put(c)
                    _check(lanes, copies, windows[win], win)
            finally:
                th.join(timeout=60)
            assert not errors, errors
        for ln in lanes:  # every launch: sources zero-copy from one chunk, outputs stored directly
            assert ln.infos == [dict(launches=w + 1, src_zero_copy=1, out_direct=1, chunks=1, records=BATCH * NBATCHES)
                                for w in range(NWIN)], (ln.name, ln.infos)
    finally:
        for ln in lanes:
            ln.stager.close()
        for cont in containers:
            for bufs in cont.values():
                for bf in bufs:
                    bf.free()
        ctx.close()


def _ramp_image(w, h, seed):
    """Constant rows plus a per-row ramp: cheap to make at 35 MB, and no two rows or columns of a crop alike."""
    y = (np.arange(h, dtype=np.uint32) * 7 + seed)[:, None, None]
    x = (np.arange(w, dtype=np.uint32) * 3)[None, :, None]
    c = (np.arange(3, dtype=np.uint32) * 85)[None, None, :]
    return ((y + x + c) & 0xFF).astype(np.uint8)


def test_two_chunk_window_then_small():
    ctx = A.Context(0)
    out = A.out_desc(channels=3, channel_major=True, bgr_to_rgb=True, dtype="float32", mean=C.MEAN, stddev=C.STDDEV,
                     item_stride=3 * 32 * 32 * 4)
    st = A.Stager(ctx, out, 2)
    buf = Buffer(2 * out.item_stride, "pinned")
    W, Hh = 3400, 3432  # 35 006 400 bytes a record: the second does not fit the first 64 MB chunk
    corners = [(W - 64, Hh - 64), (W - 64 - 1, Hh - 64 - 3)]  # 64x64 at the far corner of each record
    try:
        for step, (kind, seed) in enumerate([("large", 1), ("small", 2), ("large", 3)]):
            if kind == "large":
                imgs = [_ramp_image(W, Hh, seed * 31 + i * 101) for i in range(2)]
                params = [A.aug_params(crop_x=x, crop_y=y, crop_w=64, crop_h=64, out_w=32, out_h=32) for x, y in corners]
            else:
                imgs = [A.synthetic_image(70 + i, 100 + i, 80, 3) for i in range(2)]
                params = [A.aug_params(crop_x=3, crop_y=2, crop_w=90, crop_h=70, out_w=32, out_h=32, flip=i) for i in range(2)]
            for i in range(2):
                st.stage(buf.ptr, i, imgs[i], params[i])
            st.flush(buf.ptr)
            info = st.last_launch()
            want_info = dict(launches=step + 1, src_zero_copy=int(kind == "small"), out_direct=1,
                             chunks=2 if kind == "large" else 1, records=2)
            assert info == want_info, (step, kind, info)
            ref = H.oracle_records(imgs, params, out)
            got = buf.bytes().view(np.float32).reshape(2, -1)
            for i in range(2):
                assert np.array_equal(got[i], ref[i].reshape(-1)), (step, kind, i)
    finally:
        st.close()
        buf.free()
        ctx.close()
