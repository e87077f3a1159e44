"""Every output size through the tile, gather, records and resize kernels, bit for bit against the oracle.

The rest of the suite tests a few dozen hand-picked sizes; here the geometry of a record is swept
(tests/size_cases.py, whose docstring lists what the geometry decides on the device): every output width from 1
to 528 and eight around each later threshold of the workgroup shape, every output height from 1 to 136 at four
widths, and for CUBIC / LANCZOS4 / INTER_AREA every width from 1 to 360 and around the second band edge (one
channel: around 1024), each with crops from a third of the output to 7.3 times it, at every byte alignment of
the crop in its row, touching the source's last column and last row.

One call per width (per output size for the height sweep; per INTER_AREA class and per output size where the
form under test needs it), so the launch shapes are that width's own.  Every call writes into a buffer
pre-filled with 0xAB whose items lie 48 bytes further apart than the largest of them: every byte outside the
items' own extents must still be 0xAB afterwards.  synchronize raises on a device error word, a planner refusal
raises from the call.  Each test asserts from Context.kernel_times which kernels ran.

The oracle's transform of every record is computed once per (record set, parameter set) on 16 threads and shared
by the output forms; the sources stay on the device for the module's lifetime.  Measured on an MI355X: no test
above 1.8 s (the 16-bit masks and the float32 planes over the 608 widths), most under 0.5 s, the module 15 s
("Record sizes, swept", has each test's time, what the sweep found and what two planted
arithmetic changes did to it).
"""
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aeon_amd as A
import oracle as O
from aeon_amd import configs as C
from tests import half_ref
from tests import helpers as H
from tests import size_cases as S

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
CHUNK_BYTES, CHUNK_CALLS = 96 << 20, 64  # output buffer and calls per synchronize
GUARD = 0xAB

LIGHT = dict(lighting=[0.05, -0.08, 0.03], color_noise_std=0.1)
PHOTO = dict(brightness=0.8, saturation=1.6, hue=-12, **LIGHT)
CONTRAST = dict(brightness=0.8, saturation=1.6, hue=-12, contrast=0.7, **LIGHT)

Form = namedtuple("Form", "cn bits out photo mask ctx short")
_STD = dict(bgr_to_rgb=True, mean=C.MEAN, stddev=C.STDDEV)


def form(cn=3, bits=8, photo=None, mask=False, ctx="default", short=False, **out):
    return Form(cn, bits, dict(channels=cn, **out), photo or {}, mask, ctx, short)


FORMS = {
    "f32_chw": form(channel_major=True, dtype="float32", **_STD),
    "f16_chw": form(channel_major=True, dtype="float16", **_STD),
    "u8_hwc": form(channel_major=False, dtype="uint8"),
    "u8_chw": form(channel_major=True, dtype="uint8"),
    "gray_u8": form(cn=1, channel_major=True, dtype="uint8"),
    "mask_u8": form(cn=1, mask=True, channel_major=True, dtype="uint8"),
    "mask_u16": form(cn=1, bits=16, mask=True, channel_major=True, dtype="uint16"),
    "photo": form(photo=PHOTO, channel_major=True, dtype="float32", **_STD),
    "contrast_two_launch": form(photo=CONTRAST, ctx="two_launch", channel_major=True, dtype="float32", **_STD),
    "contrast_records": form(photo=CONTRAST, channel_major=True, dtype="float32", **_STD),
    "resize_short": form(short=True, channel_major=False, dtype="uint8"),
}
METHODS = {"CUBIC": A.INTERP_CUBIC, "AREA": A.INTERP_AREA, "LANCZOS4": A.INTERP_LANCZOS4}
METHOD_FORMS = {
    "final_f32": form(channel_major=True, dtype="float32", **_STD),
    "scratch_u8": form(photo=dict(brightness=0.9), channel_major=False, dtype="uint8"),
}


@pytest.fixture(scope="module")
def ctxs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    made = {"default": A.Context(0)}
    os.environ["AEON_HIP_RECORDS"] = "0"
    try:
        made["two_launch"] = A.Context(0)  # the flag is read when a context is created
    finally:
        del os.environ["AEON_HIP_RECORDS"]
    for c in made.values():
        c.set_timing(1)
    yield made
    for c in made.values():
        c.close()
    FAMILIES.clear()
    REF.clear()


# ---- record sets: their sources on the host and (once used) on the device ---------------------------------------
def pool_map(fn, items):
    if THREADS == 1:
        return [fn(i) for i in items]
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items, chunksize=max(1, min(64, len(items) // (4 * THREADS) or 1))))


class Family:
    """The calls ((label, records) each) of one sweep with sources of cn channels and `bits` bits per element."""

    def __init__(self, calls, cn, bits):
        self.calls, self.cn, self.bits = calls, cn, bits
        keys = list({(r.image, r.src_w, r.src_h): None for _, recs in calls for r in recs})
        eb = bits // 8

        def make(k):
            img = A.synthetic_image(k[0], k[1], k[2], cn)
            if bits == 16:  # 16-bit masks: a second image as the high byte
                img = (A.synthetic_image(k[0] + (1 << 24), k[1], k[2], cn).astype(np.uint16) << 8) | img
            return img

        self.host = dict(zip(keys, pool_map(make, keys)))
        self.desc, off = {}, 0
        for k in keys:
            self.desc[k] = A.ImgDesc(offset=off, width=k[1], height=k[2], stride=k[1] * cn * eb, channels=cn,
                                     elem_bytes=eb if bits == 16 else 0)
            off += (k[1] * k[2] * cn * eb + 15) // 16 * 16
        self.arena = np.empty(off, np.uint8)
        for k in keys:
            b = self.host[k].view(np.uint8).reshape(-1)
            self.arena[self.desc[k].offset:self.desc[k].offset + b.size] = b
        self.dev = None

    def device(self):
        import torch
        if self.dev is None:
            self.dev = torch.from_numpy(self.arena).to("cuda")
        return self.dev

    def src(self, r):
        return self.host[(r.image, r.src_w, r.src_h)]

    def descs(self, recs):
        return (A.ImgDesc * len(recs))(*[self.desc[(r.image, r.src_w, r.src_h)] for r in recs])


FAMILIES = {}


def width_calls(cn):
    return [(f"w={w}", S.width_records(w, cn)) for w in S.WIDTHS]


def height_calls(cn):
    return [(f"w={w} h={oh}", S.height_records(w, oh, cn)) for w in S.HEIGHT_WIDTHS for oh in S.HEIGHTS]


def method_calls(cn):
    return [(f"w={w}", S.method_records(w, cn)) for w in (S.METHOD_WIDTHS if cn == 3 else S.METHOD_WIDTHS_GRAY)]


def family(sweep, cn, bits=8):
    key = (sweep, cn, bits)
    if key not in FAMILIES:
        FAMILIES[key] = Family({"width": width_calls, "height": height_calls, "method": method_calls}[sweep](cn), cn, bits)
    return FAMILIES[key]


# ---- parameters and the shared reference ----------------------------------------------------------------------
def short_size(r):
    """A resize_short_size above the source's short side: the pre-pass upscales, so the cropbox still fits."""
    s = min(r.src_w, r.src_h)
    return s + max(1, s // 4)


def params_of(r, f, interp=A.INTERP_LINEAR):
    kw = dict(f.photo) if r.cn == 3 else {}  # (photometric stages need three channels)
    if f.short:
        kw["resize_short_size"] = short_size(r)
    return A.aug_params(crop_x=r.crop_x, crop_y=r.crop_y, crop_w=r.crop_w, crop_h=r.crop_h, out_w=r.out_w, out_h=r.out_h,
                        flip=r.flip, interp=interp, **kw)


REF = {}  # (sweep, cn, bits, parameter key) -> {record: the oracle's transform (uint8 / uint16 HWC)}, read-only


def transforms(fam, sweep, f, interp=A.INTERP_LINEAR):
    key = (sweep, fam.cn, fam.bits, tuple(sorted((k, str(v)) for k, v in f.photo.items())), f.short, f.mask, interp)
    if key not in REF:
        def one(call):
            res = []
            for r in call[1]:
                q, src = H.to_oracle_params(params_of(r, f, interp)), fam.src(r)
                if not f.mask:
                    t = O.transform_image(src, q)
                elif fam.bits == 8:
                    t = O.transform_mask(src, q)[:, :, None]
                else:  # NEAREST is a pure gather: the low and the high byte planes, recombined
                    lo, hi = (O.transform_mask((src >> s & 0xFF).astype(np.uint8), q) for s in (0, 8))
                    t = (hi.astype(np.uint16) << 8 | lo)[:, :, None]
                res.append((r, t))
            return res
        REF[key] = {r: t for res in pool_map(one, fam.calls) for r, t in res}
    return REF[key]


def loaded(t, f):
    """The loader's item of the transformed record t, as the bytes the device must write."""
    if t.dtype == np.uint16:  # pixel_mask's loader: convertTo, no layout change for one channel
        return np.ascontiguousarray(t.transpose(2, 0, 1))
    o = f.out
    half = o["dtype"] == "float16"
    lc = O.load_config(o["channels"], o["channel_major"], o.get("bgr_to_rgb", False), "float32" if half else o["dtype"],
                       o.get("mean"), o.get("stddev"))
    x = O.load_image(t, lc)
    return half_ref.f16_bits(x) if half else x


# ---- the runner --------------------------------------------------------------------------------------------------
def item_bytes(r, f):
    return r.out_w * r.out_h * r.cn * np.dtype(A.DTYPES[f.out["dtype"]][1]).itemsize


def where_report(r, f, got, ref, band_rows):
    """Where the elements that differ lie: the first one, their count, and how many sit in the row's last four
    columns, on the last row of a tile (band_rows rows) or of the record, and at or past the scalar-tail boundary
    (in the unflipped row's element order)."""
    g, w = (np.asarray(a).reshape(ref.shape) for a in (got, ref))
    bad = np.argwhere(g != w)
    if f.out["channel_major"]:
        c, y, x = bad[:, 0], bad[:, 1], bad[:, 2]
    else:
        y, x, c = bad[:, 0], bad[:, 1], bad[:, 2]
    if f.out.get("bgr_to_rgb"):
        c = r.cn - 1 - c
    xs = r.out_w - 1 - x if r.flip else x
    xv = S.simd_boundary(r.out_w * r.cn)
    at = tuple(int(v) for v in bad[0])
    return (f"{len(bad)} of {w.size} elements differ, first at {at}: hip={g[at]} ref={w[at]}; "
            f"{int(np.sum(x >= r.out_w - 4))} in the last four columns, "
            f"{int(np.sum((y % band_rows == band_rows - 1) | (y == r.out_h - 1)))} on the last row of a {band_rows}-row tile, "
            f"{int(np.sum(xs * r.cn + c >= xv))} at or past the scalar-tail boundary (element {xv} of {r.out_w * r.cn})")


def run_calls(ctx, fam, calls, f, ref, interp=A.INTERP_LINEAR):
    """The calls through ctx, each into its own stretch of a 0xAB buffer with item_stride = the call's largest
    item rounded up to 16, plus 48.  Returns ({'augment' | 'stats' | 'pre': launches}, failures): a failure is
    (call label, text) for an item that differs from the oracle or a guard byte that changed."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    src = fam.device()
    fn = ctx.mask_batch if f.mask else ctx.augment_batch
    failures = []
    ctx.kernel_times()  # (clears the counts)
    counts = {"augment": 0, "stats": 0, "pre": 0}
    chunks, used = [[]], 0  # of (label, records, item_stride, offset in the chunk's buffer)
    for label, recs in calls:
        stride = (max(item_bytes(r, f) for r in recs) + 15) // 16 * 16 + 48
        if used and (used + stride * len(recs) > CHUNK_BYTES or len(chunks[-1]) == CHUNK_CALLS):
            chunks.append([])
            used = 0
        chunks[-1].append((label, recs, stride, used))
        used += stride * len(recs)
    for chunk in chunks:
        size = chunk[-1][3] + chunk[-1][2] * len(chunk[-1][1])
        dst = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
        for label, recs, stride, off in chunk:
            out = A.out_desc(item_stride=stride, **f.out)
            fn(fam.descs(recs), src.data_ptr(), [params_of(r, f, interp) for r in recs], out, dst.data_ptr() + off, stream)
        ctx.synchronize(stream)
        t = ctx.kernel_times()
        for k in counts:
            counts[k] += t[k][2]
        host = dst.cpu().numpy()
        for label, recs, stride, off in chunk:
            for i, r in enumerate(recs):
                want = loaded(ref[r], f)
                at = off + i * stride
                got = host[at:at + want.nbytes]
                if not np.array_equal(got, want.view(np.uint8).reshape(-1)):
                    same = [q for q in recs if S.kind(q) == S.kind(r)]
                    tr = S.tile_rows(same, f.mask)[0]
                    failures.append((label, f"{label} record {i} {r._asdict()} {params_of(r, f, interp).as_dict()}: " +
                                     where_report(r, f, got.view(want.dtype), want, tr)))
                got[:] = GUARD
            if not np.all(host[off:off + stride * len(recs)] == GUARD):
                dirty = np.nonzero(host[off:off + stride * len(recs)] != GUARD)[0]
                i, b = divmod(int(dirty[0]), stride)
                failures.append((label, f"{label}: {dirty.size} guard bytes written, first {b - item_bytes(recs[i], f)} bytes "
                                        f"past the end of record {i} {recs[i]._asdict()} (item stride {stride})"))
        del dst
    return counts, failures


def assert_clean(failures, what):
    if failures:
        labels = list(dict.fromkeys(label for label, _ in failures))
        raise AssertionError(f"{what}: {len(failures)} failures in {len(labels)} calls ({', '.join(labels[:40])}"
                             f"{' ...' if len(labels) > 40 else ''}); the first three:\n" +
                             "\n".join(text for _, text in failures[:3]))


def contrast_record_calls(fam):
    """The contrast_records form: widths the records kernel can hold (a multiple of 4, at most 256), the
    records of a call of one output size (the kernel takes no other call).  Returns (calls the restated
    run_records says the kernel takes, the others -- a scalar row tail at widths that are no multiple of 16,
    the exact 2x records, staged rows past the LDS -- which take the two-launch path)."""
    taken, other = [], []
    for label, recs in fam.calls:
        if recs[0].out_w % 4 or recs[0].out_w > 256:
            continue
        groups = {}
        for r in recs:
            groups.setdefault((r.out_h, S.kind(r) == S.AREA2X), []).append(r)
        for (oh, _), g in groups.items():
            if S.records_kernel_takes(g) or len(g) == 1:
                (taken if S.records_kernel_takes(g) else other).append((f"{label} out_h={oh}", g))
                continue
            for r in g:  # (a call the kernel refuses for one record's staged rows: each record on its own)
                (taken if S.records_kernel_takes([r]) else other).append((f"{label} out_h={oh} crop_w={r.crop_w}", [r]))
    return taken, other


def sweep(ctxs, kind, name):
    f = FORMS[name]
    fam = family(kind, f.cn, f.bits)
    ref = transforms(fam, kind, f)
    ctx = ctxs[f.ctx]
    calls = fam.calls
    if name == "contrast_records":
        taken, other = contrast_record_calls(fam)
        assert len(taken) >= (16 if kind == "width" else 200) and other
        counts, failures = run_calls(ctx, fam, taken, f, ref)
        assert_clean(failures, f"{kind} sweep, {name}: the records kernel")
        assert counts == {"augment": len(taken), "stats": 0, "pre": 0}, counts
        counts, failures = run_calls(ctx, fam, other, f, ref)
        assert_clean(failures, f"{kind} sweep, {name}: calls the records kernel does not take")
        assert counts["stats"] >= len(other), counts
        return
    counts, failures = run_calls(ctx, fam, calls, f, ref)
    assert_clean(failures, f"{kind} sweep, {name}")
    n = len(calls)
    if f.mask:  # the gather pass: one launch per call
        assert counts == {"augment": n, "stats": 0, "pre": 0}, counts
    elif name == "contrast_two_launch":  # KM_STATS, contrast_reduce, KM_FINAL for every call
        assert counts["stats"] >= n and counts["augment"] >= n, counts
    elif name == "resize_short":  # the KM_RAW pre-pass of every call
        assert counts["pre"] >= n and counts["stats"] == 0 and counts["augment"] >= n, counts
    elif name == "photo":  # (pre: the exact 2x records resize ahead of their photometric copy pass)
        assert counts["stats"] == 0 and counts["pre"] >= n and counts["augment"] >= n, counts
    else:  # the tile kernel alone, one launch per (resize mode, scalar tail) group of a call
        assert counts["stats"] == 0 and counts["pre"] == 0 and counts["augment"] >= n, counts
        if kind == "width":  # identity + linear records, and the 2x record, are two groups at least
            assert counts["augment"] >= 2 * n, counts


@pytest.mark.parametrize("name", list(FORMS))
def test_width_sweep(ctxs, name):
    """Every width of size_cases.WIDTHS, one call per width, through the form `name`."""
    sweep(ctxs, "width", name)


@pytest.mark.parametrize("name", list(FORMS))
def test_height_sweep(ctxs, name):
    """Every height of size_cases.HEIGHTS at four widths, one call per output size, through the form `name`."""
    sweep(ctxs, "height", name)


@pytest.mark.parametrize("name", list(METHOD_FORMS))
@pytest.mark.parametrize("method", list(METHODS))
def test_method_sweep(ctxs, method, name):
    """CUBIC / LANCZOS4 / INTER_AREA at every width of size_cases.METHOD_WIDTHS (three channels) and
    METHOD_WIDTHS_GRAY (one).  final_f32: no photometric stage, float32 planes: the resize pass writes the
    loader's item itself (pre launches only, but for INTER_AREA's integer boxes, which always go through
    scratch and a copy pass).  scratch_u8: a brightness stage (three channels) and uint8 HWC output: the
    resize pass writes scratch and the tile kernel's copy pass follows.  INTER_AREA: a call per class of a
    width's records (a launch takes the class of its most taps)."""
    f3 = METHOD_FORMS[name]
    f1 = f3._replace(cn=1, photo={}, out=dict({k: v for k, v in f3.out.items() if k not in ("bgr_to_rgb", "mean", "stddev")},
                                              channels=1, **(dict(mean=[0.5], stddev=[0.25]) if "mean" in f3.out else {})))
    interp = METHODS[method]
    for f in (f3, f1):
        fam = family("method", f.cn)
        ref = transforms(fam, "method", f, interp)
        calls = fam.calls
        if method == "AREA":
            calls = []
            for label, recs in fam.calls:
                groups = {}
                for r in recs:
                    groups.setdefault(S.area_class(r.crop_w, r.crop_h, r.out_w, r.out_h), []).append(r)
                calls += [(f"{label} {cls}", g) for cls, g in groups.items()]
        counts, failures = run_calls(ctxs["default"], fam, calls, f, ref, interp)
        assert_clean(failures, f"method sweep, {method} {name}, {f.cn} channels")
        resized = [c for c in calls if method != "AREA" or c[0].split()[-1] not in (S.IDENTITY, S.AREA_2X)]
        assert counts["pre"] >= len(resized) > 0 and counts["stats"] == 0, counts
        if name == "scratch_u8":
            assert counts["augment"] >= len(calls), counts
        elif method != "AREA":
            assert counts["augment"] == 0, counts
