"""Every BGR triple through every kernel form of the photometric stages, bit for bit against the oracle.

The stages of augment_device.hpp (bs_apply, hue_apply_n, hue_pack_n) rest on claims over all 2^24 colours
(v / 255 * 255 rounds back to v, no product leaves [0, 255], cvt_pk_u8_f32 + v_perm reproduce u8rnd in every
HSV sector, the 10-bit fixed-point transform is exact in any order).  The rest of the suite feeds them
synthetic noise that a bilinear resize has pulled towards grey; here the input is the colour cube itself
(tests/colour_cases.py), cut into identity records -- crop = record = output, so the resize is a copy and the
pixels entering the stages are exactly the cube -- and sent through each form:

  1. the tile kernel in one pass (photometric without contrast, uint8 HWC), its jobs read from the caller's
     pinned slot (the default context) and from the device job table (AEON_HIP_DIRECT=0);
  2. the two-launch contrast path: pass 1 (its specialised loop, hue_pack_n, for fixed-point
     brightness/saturation with a hue shift; the generic loop otherwise), contrast_reduce, pass 2
     (RESIZE_COPY + photometric);
  3. the records kernel (contrast records in one launch, float32 CHW with mean/stddev): its FAST form (every
     record fixed point) and its GENERIC one, also against the two-launch path (AEON_HIP_RECORDS=0);
  4. a resize pre-pass into scratch + the tile kernel's RESIZE_COPY + photometric form without contrast.  An
     identity record never takes it, whatever its interpolation (the planner sends a same-size CUBIC record
     through the tile kernel's identity taps: asserted below); the 2x INTER_AREA pre-pass of a record with
     every pixel doubled both ways does, and hands the copy pass the cube ((4 v + 2) >> 2 = v).

Each test asserts from Context.kernel_times launch counts that the form it names is the one that ran; which
loop a launch takes inside the kernel follows from the record's cv::transform class, restated here (bs_kind).
A 256 x 250 lattice record of 40 levels per channel goes through forms 1 and 2 at every hue in [-180, 180]
and at -397 and 401 (the per-tile hue table is built on the device for each hue).

The oracle's output is computed once per parameter set and record shape (REF) and shared by the forms.
Reference time, measured on the GPU machine's CPUs (16 oracle threads): the slowest parameter set, the full
chain with contrast over the 16 slabs, takes 0.03-0.04 s (0.22 s on 8 threads of a slower CPU); the whole
module runs in 4 s, no test in more than 0.2 s."""
import os

import numpy as np
import pytest

import aeon_amd as A
import oracle as O
from aeon_amd import configs as C
from tests import colour_cases as K
from tests import helpers as H

pytestmark = pytest.mark.gpu

SLAB, N_SLABS = 1024, 16
REC_W, REC_H = 256, 224
N_RECS = K.cube_record_count(REC_W, REC_H)
THREADS = min(16, os.cpu_count() or 1)

LIGHT = dict(lighting=[0.05, -0.08, 0.03], color_noise_std=0.1)
# photometric parameter sets without contrast: one hue per wrap class ((H + hue) % 180 stored as uchar: no
# wrap, a negative remainder, |hue| >= 180), each cv::transform class, and the chain with C3's ranges
PLAIN = {
    "hue_7": dict(hue=7),
    "hue_m13": dict(hue=-13),
    "hue_m187": dict(hue=-187),
    "bs_diag": dict(brightness=0.6, saturation=1.0),
    "bs_fixpt": dict(brightness=0.75, saturation=1.8),
    "bs_float": dict(brightness=40.0, saturation=1.5),
    "chain": dict(brightness=0.8, saturation=1.6, hue=-12, **LIGHT),
}
# ... and with contrast: (expected pass-1 loop, params)
CONTRAST = {
    "spec": ("spec", dict(brightness=0.75, saturation=1.8, hue=11, contrast=0.65)),
    "spec_chain": ("spec", dict(brightness=0.8, saturation=1.6, hue=-12, contrast=0.7, **LIGHT)),
    "generic_diag": ("generic", dict(brightness=0.6, saturation=1.0, hue=-13, contrast=1.3)),
    "generic_float": ("generic", dict(brightness=40.0, saturation=1.5, contrast=0.8)),
}
SATURATING = ("bs_fixpt", "bs_float")  # sets that must clip at both ends of the cube
SWEEP_HUES = list(range(-180, 181)) + [-397, 401]

BS_DIAG, BS_FIXPT, BS_FLOAT = "diag", "fixpt", "float"


def bs_kind(brightness, saturation):
    """The cv::transform OpenCV 2.4 picks for cbsjitter's matrix (plan_bs, plan_record.hpp), restated."""
    f = np.float32
    g = [f(0.0820), f(0.6094), f(0.3086)]
    b, s = f(brightness), f(saturation)
    oms = f(f(1) - s)
    M = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            a = s if i == j else f(0)
            bb = f(float(oms) * float(g[j]))
            M[i, j] = f(a + bb) if b == f(1) else f(float(a) * float(b) + float(bb) * float(b) + 0.0)
    off = M[~np.eye(3, dtype=bool)]
    if np.all(np.abs(off.astype(np.float64)) <= np.finfo(np.float32).eps):
        return BS_DIAG
    return BS_FIXPT if np.all(np.abs(M) < 32) else BS_FLOAT


def test_parameter_sets_cover_the_transform_classes():
    kinds = {k: bs_kind(p.get("brightness", 1.0), p.get("saturation", 1.0)) for k, p in PLAIN.items() if k.startswith("bs_")}
    assert kinds == {"bs_diag": BS_DIAG, "bs_fixpt": BS_FIXPT, "bs_float": BS_FLOAT}
    for name, (loop, p) in CONTRAST.items():
        spec = bs_kind(p["brightness"], p["saturation"]) == BS_FIXPT and p.get("hue", 0) != 0 and SLAB % 4 == 0
        assert spec == (loop == "spec"), name


# ---- contexts, device-resident inputs, the shared reference --------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    made = {"default": A.Context(0)}
    for name, flag in (("table", "AEON_HIP_DIRECT"), ("two_launch", "AEON_HIP_RECORDS")):
        os.environ[flag] = "0"
        try:
            made[name] = A.Context(0)  # the flags are read when a context is created
        finally:
            del os.environ[flag]
    for c in made.values():
        c.set_timing(1)
    yield made
    for c in made.values():
        c.close()


class Inputs:
    """Record sets kept on the host and (once used) on the device for the module's lifetime."""

    def __init__(self):
        self.host, self.dev = {}, {}

    def images(self, kind):
        if kind not in self.host:
            if kind == "slabs":
                self.host[kind] = K.cube_records(SLAB, SLAB)
            elif kind == "slabs_2x":
                self.host[kind] = [np.repeat(np.repeat(s, 2, axis=0), 2, axis=1) for s in self.images("slabs")]
            elif kind == "records":
                self.host[kind] = K.cube_records(REC_W, REC_H)
            else:
                self.host[kind] = [K.lattice_record()]
        return self.host[kind]

    def device(self, kind):
        import torch
        if kind not in self.dev:
            arena, descs = A.pack_images(self.images(kind))
            self.dev[kind] = (torch.from_numpy(arena).to("cuda"), descs)
        return self.dev[kind]


@pytest.fixture(scope="module")
def inputs():
    inp = Inputs()
    yield inp
    inp.dev.clear()


REF = {}        # (record set, output form, parameter key) -> the oracle's outputs, read-only
REF_SECS = {}   # ... and the oracle's own time for them

U8_HWC = dict(channels=3, channel_major=False, dtype="uint8")
F32_CHW = dict(channels=3, channel_major=True, bgr_to_rgb=True, dtype="float32", mean=C.MEAN, stddev=C.STDDEV)


def identity(w, h, **photo):
    return A.aug_params(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=w, out_h=h, **photo)


def reference(key, images, params, out, shape):
    if key not in REF:
        res, secs = O.batch_augment(images, [H.to_oracle_params(p) for p in params], H.oracle_load_config(out), shape,
                                    THREADS)
        res.setflags(write=False)
        REF[key], REF_SECS[key] = res, secs
        print(f"[reference {key}: {secs:.3f} s on {THREADS} threads]")
    return REF[key]


def slab_reference(inputs, name, photo):
    imgs = inputs.images("slabs")
    out = A.out_desc(item_stride=SLAB * SLAB * 3, **U8_HWC)
    return reference(("slabs", name), imgs, [identity(SLAB, SLAB, **photo)] * len(imgs), out, (SLAB, SLAB, 3))


def run(ctx, src, descs, params, out, shape, dtype=np.uint8, chunk=None):
    """The records through ctx.augment_batch, `chunk` per call, into a buffer pre-filled with 0xAB; returns
    (outputs (n, *shape), {'augment' | 'stats' | 'pre': launches}).  synchronize raises on a device error word."""
    import torch
    n = len(params)
    chunk = chunk or n
    assert out.item_stride == int(np.prod(shape)) * np.dtype(dtype).itemsize
    dst = torch.full((n * out.item_stride,), 0xAB, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.kernel_times()  # (clears the counts)
    for i in range(0, n, chunk):
        ctx.augment_batch(descs[i:i + chunk], src.data_ptr(), params[i:i + chunk], out,
                          dst.data_ptr() + i * out.item_stride, stream)
    ctx.synchronize(stream)
    t = ctx.kernel_times()
    return dst.cpu().numpy().view(dtype).reshape((n,) + tuple(shape)), {k: t[k][2] for k in ("augment", "stats", "pre")}


def assert_same(got, ref, what, src=None):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if np.array_equal(got, ref):
        return
    bad = np.argwhere(got != ref)
    at = tuple(bad[0])
    msg = f"{what}: {len(bad)} values differ, first at {at}: hip={got[at]} ref={ref[at]}"
    if src is not None:  # HWC uint8 outputs of identity records: the input colour
        msg += f", input BGR {tuple(int(v) for v in src[at[0]][at[1], at[2]])}"
    raise AssertionError(msg)


# ---- the geometry hands the stages the cube ------------------------------------------------------------------
def test_identity_records_are_the_cube_on_the_device(ctxs, inputs):
    """No photometric stage: the device's output of the identity records is the cube itself (slabs, records
    and lattice)."""
    for kind, w, h, chunk in (("slabs", SLAB, SLAB, 8), ("records", REC_W, REC_H, 64), ("lattice", K.LATTICE_W, K.LATTICE_H, 1)):
        imgs = inputs.images(kind)
        src, descs = inputs.device(kind)
        out = A.out_desc(item_stride=w * h * 3, **U8_HWC)
        got, counts = run(ctxs["default"], src, descs, [identity(w, h)] * len(imgs), out, (h, w, 3), chunk=chunk)
        assert counts == {"augment": (len(imgs) + chunk - 1) // chunk, "stats": 0, "pre": 0}
        assert_same(got, np.stack(imgs), kind + " identity")


# ---- form 1: the tile kernel, one pass ------------------------------------------------------------------------
@pytest.mark.parametrize("jobs", ["default", "table"])
@pytest.mark.parametrize("name", list(PLAIN))
def test_tile_kernel_single_pass(ctxs, inputs, name, jobs):
    """Form 1: photometric without contrast, uint8 HWC, one launch per call of 8 slabs (a call's 8 x 128 job
    reads stay well inside what run_direct takes), jobs from the pinned slot or the device table."""
    photo = PLAIN[name]
    ref = slab_reference(inputs, name, photo)
    imgs = inputs.images("slabs")
    if name in SATURATING:  # clips at both ends, in channels that were at neither
        cube = np.stack(imgs)
        inside = (cube != 0) & (cube != 255)
        assert np.any((ref == 0) & inside) and np.any((ref == 255) & inside)
    src, descs = inputs.device("slabs")
    out = A.out_desc(item_stride=SLAB * SLAB * 3, **U8_HWC)
    got, counts = run(ctxs[jobs], src, descs, [identity(SLAB, SLAB, **photo)] * N_SLABS, out, (SLAB, SLAB, 3), chunk=8)
    assert counts == {"augment": 2, "stats": 0, "pre": 0}
    assert_same(got, ref, f"single pass {name} ({jobs} jobs)", imgs)


# ---- form 2: the two-launch contrast path ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONTRAST))
def test_two_launch_contrast_path(ctxs, inputs, name):
    """Form 2: 1024-row records are too tall for the records kernel, so a contrast call takes pass 1 (one stats
    launch: the specialised loop for fixed-point brightness/saturation + hue, else the generic one),
    contrast_reduce and pass 2 (one augment launch, RESIZE_COPY + photometric)."""
    _, photo = CONTRAST[name]
    ref = slab_reference(inputs, name, photo)
    src, descs = inputs.device("slabs")
    out = A.out_desc(item_stride=SLAB * SLAB * 3, **U8_HWC)
    got, counts = run(ctxs["default"], src, descs, [identity(SLAB, SLAB, **photo)] * N_SLABS, out, (SLAB, SLAB, 3))
    assert counts == {"augment": 1, "stats": 1, "pre": 0}
    assert_same(got, ref, f"two-launch {name}", inputs.images("slabs"))


# ---- form 3: the records kernel -------------------------------------------------------------------------------
def record_params(batch):
    spec = CONTRAST["spec"][1]
    params = [identity(REC_W, REC_H, **(dict(spec, **LIGHT) if i % 3 == 0 else spec)) for i in range(N_RECS)]
    if batch == "generic":  # a diagonal and a float cv::transform among the fixed-point records
        params[5] = identity(REC_W, REC_H, **CONTRAST["generic_diag"][1])
        params[250] = identity(REC_W, REC_H, **CONTRAST["generic_float"][1])
    return params


@pytest.mark.parametrize("batch", ["fast", "generic"])
def test_records_kernel(ctxs, inputs, batch):
    """Form 3: 293 records of 256 x 224 hold the cube; float32 CHW with mean/stddev, contrast on every record:
    one augment launch and no stats launch on the default context (FAST: every record fixed point; GENERIC: a
    diagonal and a float record among them), and the same bytes from the two-launch path."""
    params = record_params(batch)
    kinds = {bs_kind(p.brightness, p.saturation) for p in params}
    assert kinds == ({BS_FIXPT} if batch == "fast" else {BS_FIXPT, BS_DIAG, BS_FLOAT})
    imgs = inputs.images("records")
    shape = (3, REC_H, REC_W)
    out = A.out_desc(item_stride=3 * REC_W * REC_H * 4, **F32_CHW)
    ref = reference(("records", batch), imgs, params, out, shape)
    src, descs = inputs.device("records")
    got, counts = run(ctxs["default"], src, descs, params, out, shape, np.float32)
    assert counts == {"augment": 1, "stats": 0, "pre": 0}
    assert_same(got, ref, f"records kernel ({batch})")
    two, counts = run(ctxs["two_launch"], src, descs, params, out, shape, np.float32)
    assert counts == {"augment": 1, "stats": 1, "pre": 0}
    assert_same(two, ref, f"records through the two-launch path ({batch})")


# ---- form 4: a resize pre-pass + the copy pass ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "bs_float"])
def test_prepass_then_copy_pass(ctxs, inputs, name):
    """Form 4: every slab with its pixels doubled both ways, 2048 x 2048 -> 1024 x 1024: the 2x INTER_AREA
    pre-pass (a pre launch) leaves the slab in scratch, and the tile kernel's RESIZE_COPY + photometric form
    (an augment launch) takes it from there.  The oracle on the doubled slab gives the identity record's output
    (checked on the first slab), so the reference is the shared one."""
    photo = PLAIN[name]
    ref = slab_reference(inputs, name, photo)
    twice = inputs.images("slabs_2x")
    p = A.aug_params(crop_x=0, crop_y=0, crop_w=2 * SLAB, crop_h=2 * SLAB, out_w=SLAB, out_h=SLAB, **photo)
    out = A.out_desc(item_stride=SLAB * SLAB * 3, **U8_HWC)
    (first,) = H.oracle_records(twice[:1], [p], out)
    assert np.array_equal(first, ref[0])
    src, descs = inputs.device("slabs_2x")
    got, counts = run(ctxs["default"], src, descs, [p] * N_SLABS, out, (SLAB, SLAB, 3))
    assert counts == {"augment": 1, "stats": 0, "pre": 1}
    assert_same(got, ref, f"pre-pass + copy pass {name}", inputs.images("slabs"))


def test_cubic_identity_records_take_the_tile_kernel(ctxs, inputs):
    """A same-size record is a copy under every interpolation (image::resize's shortcut), and the planner sends
    a CUBIC one with photometric stages through the tile kernel's identity taps, from the device job table: one
    augment launch, no pre launch -- the same bytes as form 1."""
    photo = PLAIN["chain"]
    ref = slab_reference(inputs, "chain", photo)
    src, descs = inputs.device("slabs")
    out = A.out_desc(item_stride=SLAB * SLAB * 3, **U8_HWC)
    params = [identity(SLAB, SLAB, interp=A.INTERP_CUBIC, **photo)] * N_SLABS
    got, counts = run(ctxs["default"], src, descs, params, out, (SLAB, SLAB, 3))
    assert counts == {"augment": 1, "stats": 0, "pre": 0}
    assert_same(got, ref, "CUBIC identity", inputs.images("slabs"))


# ---- every hue on the lattice -----------------------------------------------------------------------------------
def sweep(ctxs, inputs, name, photo, chunk, expect):
    w, h = K.LATTICE_W, K.LATTICE_H
    n = len(SWEEP_HUES)
    imgs = inputs.images("lattice") * n
    params = [identity(w, h, hue=hue, **photo) for hue in SWEEP_HUES]
    out = A.out_desc(item_stride=w * h * 3, **U8_HWC)
    ref = reference(("lattice", name), imgs, params, out, (h, w, 3))
    src, descs = inputs.device("lattice")
    got, counts = run(ctxs["default"], src, list(descs) * n, params, out, (h, w, 3), chunk=chunk)
    assert counts == expect
    for i, hue in enumerate(SWEEP_HUES):
        assert_same(got[i:i + 1], ref[i:i + 1], f"{name} hue {hue}", imgs)


def test_hue_sweep_single_pass(ctxs, inputs):
    """Form 1 at every hue in [-180, 180], -397 and 401: one lattice record per hue, 128 records per call.  One
    launch per call, but for the call that holds the hue-0 record: that record has no photometric stage, so the
    call goes through the planner as two launch groups (with and without photometric stages)."""
    assert 128 <= SWEEP_HUES.index(0) < 256
    sweep(ctxs, inputs, "hue sweep", {}, 128, {"augment": 4, "stats": 0, "pre": 0})


def test_hue_sweep_specialised_contrast_loop(ctxs, inputs):
    """Form 2's specialised pass-1 loop (hue_pack_n) at every hue (the hue-0 record, with no hue stage, takes the
    generic loop): a 250-row record is too tall for the records kernel."""
    assert bs_kind(0.75, 1.8) == BS_FIXPT and K.LATTICE_W % 4 == 0
    sweep(ctxs, inputs, "spec hue sweep", dict(brightness=0.75, saturation=1.8, contrast=0.65), None,
          {"augment": 1, "stats": 1, "pre": 0})
