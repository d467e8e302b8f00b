"""pt_present_set_arithmetic(h, PT_ARITH_REFERENCE) on the GPU: pt_postprocess_reference_kernel (csrc/pt_integrate_reference.hip,
csrc/pt_postprocess_reference.hpp) tone-maps every present that follows with llvmpipe's arithmetic choices.  "The host" below is the same
header compiled for the CPU (tests/postprocess_probe.py), which tests/test_reference_postprocess_cpu.py pins to the reference's own float
colours bit for bit; the contract side is the oracle, as everywhere.  Images are loaded with pt_write_result unless frames are rendered."""
import numpy as np
import pytest

import configs
import fixtures
import postprocess_probe as probe
from test_gpu_abi_round2 import make_tracer
from test_gpu_round6 import _Tune

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_image(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    if not np.array_equal(got, want):
        bad = (got != want).any(-1)
        first = np.argwhere(bad)[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {first}: got {got[tuple(first[0])].tolist()}, "
                             f"want {want[tuple(first[0])].tolist()}")


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return probe.build(pkg, tmp_path_factory.mktemp("ppprobe"))


def loaded(pkg, image, **extra):
    """a tracer that holds `image` as its accumulation (frame counter 1)"""
    t = pkg.PathTracer(None, image.shape[1], image.shape[0], 1, 1, 1.0, 0.0, **extra)
    t.WriteResult(image, 1)
    return t


def log_uniform(h, w, seed):
    rng = np.random.default_rng(seed)
    return probe.rgba((10.0 ** rng.uniform(-5.0, 2.0, (h, w, 3))).astype(np.float32))


# ------------------------------------------------------------------------------------------------ (1) the reference's fixture
def test_fixture_in_both_modes_and_back(pkg, native_lib, oracle):
    N = pkg.native
    fx = fixtures.load("post_aces_gamma")
    img, expected = fx["image"], fx["expected"]
    assert img.shape == (96, 64, 4)
    want_ref = np.full(img.shape, 255, np.uint8)
    want_ref[..., :3] = (np.clip(expected, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)  # round-half-up of clamp * 255
    pt = loaded(pkg, img)
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    first = pt.Present()
    assert_same_image(first, want_ref, "REFERENCE present of the fixture against the reference's float colours")
    pt.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    assert_same_image(pt.Present(), oracle.postprocess(img)[1], "CONTRACT present after switching back")
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    assert_same_image(pt.Present(), first, "REFERENCE present again")
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ (2) the switch takes effect
@pytest.mark.parametrize("which", ["witness_8x8", "ramp_1024x256"])
def test_the_switch_takes_effect(pkg, native_lib, oracle, host, which):
    """The two arithmetics differ in RGBA8 on these images (by 1 LSB, at the inputs tests/test_reference_postprocess_cpu.py lists): the
    REFERENCE present is the host's, the CONTRACT present the oracle's, and they differ exactly where those two do."""
    N = pkg.native
    img = probe.witness_tile() if which == "witness_8x8" else probe.ramp()
    want_ref, want_con = host.rgba8(img), oracle.postprocess(img)[1]
    differ = want_ref != want_con
    assert differ[..., :3].all() if which == "witness_8x8" else differ.sum() == 4  # (the figures of the CPU suite)
    pt = loaded(pkg, img)
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    ref = pt.Present()
    pt.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    con = pt.Present()
    pt.Dispose()
    print(f"\n  {which}: {int((ref != con).sum())} RGBA8 values differ between the two presents (host: {int(differ.sum())})")
    assert_same_image(ref, want_ref, f"{which}: REFERENCE present against the host")
    assert_same_image(con, want_con, f"{which}: CONTRACT present against the oracle")
    assert np.array_equal(ref != con, differ)


# ------------------------------------------------------------------------------------------------ (3) sizes
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (75, 43), (1280, 820)], ids=lambda v: str(v))
def test_sizes(pkg, native_lib, host, w, h):
    """one lane; one partial workgroup; a pixel count that is no multiple of 256; more than 4096 * 256 pixels (the stride loop runs)"""
    img = log_uniform(h, w, 1000 * w + h)
    if w * h > 1:
        img[h // 2, w // 2, :3] = (0.0, -0.5, -0.001)
    pt = loaded(pkg, img)
    pt.SetPresentArithmetic(pkg.native.PT_ARITH_REFERENCE)
    got = pt.Present()
    pt.Dispose()
    assert_same_image(got, host.rgba8(img), f"{w}x{h}")


# ------------------------------------------------------------------------------------------------ (4) every present path
def witness_rows(h, w, seed):
    """log-uniform values with the four witness inputs (probe.WITNESS_BITS) in the first four pixels of EVERY row: whichever rows a part
    of a group, a stripe or a slot covers, the two arithmetics differ there"""
    img = log_uniform(h, w, seed)
    img[:, :4, :3] = np.resize(np.array(probe.WITNESS_BITS, np.uint32).view(np.float32), 12).reshape(4, 3)
    return img


def assert_discriminates(want_ref, want_con, what):
    """the expected REFERENCE image differs from the CONTRACT one in every row: a path that ran the contract kernel cannot pass"""
    rows = (want_ref != want_con).any(axis=(1, 2))
    assert rows.all(), f"{what}: host and oracle agree on rows {np.flatnonzero(~rows)[:8].tolist()}: the comparison would not tell the kernels apart"


def test_postprocess_device_and_group_handle(pkg, native_lib, oracle, host):
    torch = pytest.importorskip("torch")
    N = pkg.native
    img = witness_rows(43, 75, 7)
    want, contract = host.rgba8(img), oracle.postprocess(img)[1]
    assert_discriminates(want, contract, "75x43")
    pt = loaded(pkg, img)
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    dev = pkg.distributed.postprocessed_tile(pt).cpu().numpy()
    pt.Dispose()
    assert_same_image(dev, want, "pt_postprocess_device")
    # the group handle: the switch fans out to the parts, each part tone-maps its own rows before the gather (sync and async)
    g = loaded(pkg, img, devices=[0, 0, 0])
    assert_same_image(g.Present(), contract, "group handle over 3 parts, CONTRACT: pt_present_rgba8")
    g.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    assert_same_image(g.Present(), want, "group handle over 3 parts: pt_present_rgba8")
    g.PresentAsync(0)
    shown, idx = g.PresentWait(0)
    assert idx == 1
    assert_same_image(shown.copy(), want, "group handle over 3 parts: pt_present_rgba8_async")
    for bad in (2, -1):
        assert native_lib.pt_present_set_arithmetic(g._h, bad) == N.PT_E_BAD_ARGUMENT
    assert_same_image(g.Present(), want, "group handle: still REFERENCE after rejected modes")
    g.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    g.PresentAsync(1)
    shown, _ = g.PresentWait(1)
    assert_same_image(shown.copy(), contract, "group handle over 3 parts, back to CONTRACT: pt_present_rgba8_async")
    g.Dispose()


def test_async_presents_of_a_witness_image_on_every_slot_and_branch(pkg, native_lib, oracle, host):
    """pt_present_rgba8_async on images that tell the kernels apart in every row.  (a) A loaded image, no frame rendered: the
    accumulation-image branch behind a join, on the two pinned slots and on a slot bound to a torch tensor.  (b) Frames rendered ON TOP of
    the witness image with the frame counter at 2^30, so that a frame moves a value by 2^-30 of its distance to the new sample and most
    witness values survive: the first present follows a frame launched without a snapshot (row stripes), the ones after it present every
    frame (snapshots); the expected image is the host's tone map of pt_read_result right after the wait (no frame in between), and it is
    checked to differ from the oracle's tone map of the same floats before it is used."""
    torch = pytest.importorskip("torch")
    N = pkg.native
    w = configs.Workload("ppwit", "default", 96, 54, 4, "sky_f32_32")
    img = witness_rows(w.height, w.width, 11)
    img[..., :3] = np.resize(np.array(probe.WITNESS_BITS, np.uint32).view(np.float32), w.height * w.width * 3).reshape(w.height, w.width, 3)
    want, contract = host.rgba8(img), oracle.postprocess(img)[1]
    assert_discriminates(want, contract, "witness image")
    pt = make_tracer(pkg, w)
    first = 1 << 30
    pt.WriteResult(img, first)
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    bound = torch.zeros((w.height, w.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pt.BindPresentImage(2, bound.data_ptr(), bound.numel())

    def present(slot):
        pt.PresentAsync(slot)
        image, idx = pt.PresentWait(slot)
        return (bound.cpu().numpy().copy() if slot == 2 else image.copy()), idx

    for slot in (0, 1, 2):  # (a)
        image, idx = present(slot)
        assert idx == first
        assert_same_image(image, want, f"loaded witness image, slot {slot}")
    survived = []
    for i, slot in enumerate((0, 1, 2, 0, 1, 2)):  # (b)
        pt.Render()
        image, idx = present(slot)
        accum = pt.Result
        assert idx == first + i + 1
        want_i, contract_i = host.rgba8(accum), oracle.postprocess(accum)[1]
        assert_discriminates(want_i, contract_i, f"witness image under {i + 1} rendered frames")
        survived.append(int((want_i != contract_i).sum()))
        assert_same_image(image, want_i, f"witness image under {i + 1} rendered frames, slot {slot}")
    # back to CONTRACT on the same handle: the same floats, the oracle's image
    pt.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    image, _ = present(0)
    assert_same_image(image, oracle.postprocess(pt.Result)[1], "the same handle back in CONTRACT")
    pt.BindPresentImage(2, None)
    pt.Dispose()
    print(f"\n  RGBA8 values that tell the kernels apart: {int((want != contract).sum())} loaded, {survived} under rendered frames")


def test_async_presents_of_rendered_frames_on_all_slots(pkg, native_lib, oracle, host):
    """Render / PresentAsync through the branches of pt_present_rgba8_async: the first present follows a frame launched without a
    snapshot (row stripes or the accumulation image), the second follows no new frame (accumulation image behind a join), the loop after
    them presents every frame (snapshots); slots 0 and 1 are the library's pinned images, slot 2 is bound to a torch tensor.  Every image
    == the host's tone map of the oracle's accumulation at the frame index the library reports."""
    torch = pytest.importorskip("torch")
    w = configs.Workload("pparith", "default", 96, 54, 4, "sky_f32_32")
    sc, basic, objs, env, kw = configs.inputs(w)
    frames = 9
    acc = oracle.render(w.width, w.height, basic, objs, env, num_frames=frames, dump_each=True, **kw)
    pt = make_tracer(pkg, w)
    pt.SetPresentArithmetic(pkg.native.PT_ARITH_REFERENCE)
    bound = torch.zeros((w.height, w.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pt.BindPresentImage(2, bound.data_ptr(), bound.numel())
    shown = []

    def wait(slot):
        image, idx = pt.PresentWait(slot)
        shown.append((slot, idx, bound.cpu().numpy().copy() if slot == 2 else image.copy()))

    pt.Render()
    pt.PresentAsync(0)
    pt.PresentAsync(1)
    wait(0)
    wait(1)
    for f in range(1, frames):
        pt.Render()
        pt.PresentAsync(f % 3)
        if f >= 3:
            wait((f - 2) % 3)
    for f in (frames - 2, frames - 1):
        wait(f % 3)
    final = pt.Result
    pt.BindPresentImage(2, None)
    pt.Dispose()
    assert sorted(idx for _, idx, _ in shown) == [1] + list(range(1, frames + 1)) and {s for s, _, _ in shown} == {0, 1, 2}
    for slot, idx, image in shown:
        assert_same_image(image, host.rgba8(acc[idx - 1]), f"slot {slot}, frame {idx}")
    assert np.array_equal(bits(final), bits(acc[-1]))


def test_a_host_that_presents_every_frame_into_bound_images(pkg, native_lib, oracle, host):
    """pt_set_frame_batch(1), Render / PresentAsync into bound device images every frame, with the knobs under which the CONTRACT mode
    shows such frames through the fused display of a frame-fed launch (tests/test_gpu_round6.py): in REFERENCE mode that display is not
    used, and every image shown is the host's tone map of exactly the frame reported."""
    torch = pytest.importorskip("torch")
    w = configs.Workload("ppfed", "default", 128, 72, 4, "sky_f32_32")
    sc, basic, objs, env, kw = configs.inputs(w)
    frames = 12
    acc = oracle.render(w.width, w.height, basic, objs, env, num_frames=frames, dump_each=True, **kw)
    with _Tune(pkg, feed_min_tiles=0, feed_idle_us=20000, feed_display=1):
        pt = make_tracer(pkg, w)
        pt.SetFrameBatch(1)
        pt.SetPresentArithmetic(pkg.native.PT_ARITH_REFERENCE)
        bufs = [torch.zeros((w.height, w.width, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for s_, b_ in enumerate(bufs):
            pt.BindPresentImage(s_, b_.data_ptr(), b_.numel())
        shown = {}
        for f in range(frames):
            pt.Render()
            if f >= 2:
                _, idx = pt.PresentWait(f % 2)
                shown[idx] = bufs[f % 2].cpu().numpy().copy()
            pt.PresentAsync(f % 2)
        for s_ in ((frames - 2) % 2, (frames - 1) % 2):
            _, idx = pt.PresentWait(s_)
            shown[idx] = bufs[s_].cpu().numpy().copy()
        st = pkg.native.debug_launch_stats(pt._h)
        final = pt.Result
        for s_ in range(2):
            pt.BindPresentImage(s_, None)
        pt.Dispose()
    print(f"\n  present loop in REFERENCE mode: {st['feed_opens']} fed launches, {st['published']} frames published, {st['launches']} launches")
    assert sorted(shown) == list(range(1, frames + 1))
    # no displaying frame-fed launch took the frames: tests/test_gpu_round6.py asserts published >= frames // 2 for the same loop in
    # CONTRACT mode (only the frames before the library has seen the host present every frame may go into a fed launch, which shows nothing)
    assert st["published"] < frames // 2, st
    for idx, image in shown.items():
        assert_same_image(image, host.rgba8(acc[idx - 1]), f"presented frame {idx}")
    assert np.array_equal(bits(final), bits(acc[-1]))


# ------------------------------------------------------------------------------------------------ (5) independence
def test_the_switch_is_independent(pkg, native_lib, oracle, host):
    N = pkg.native
    w = configs.Workload("ppindep", "default", 64, 40, 4, "sky_f32_32")
    sc, basic, objs, env, kw = configs.inputs(w)
    acc = oracle.render(w.width, w.height, basic, objs, env, num_frames=8, dump_each=True, **kw)
    pt = make_tracer(pkg, w)
    for _ in range(3):
        pt.Render()
    before = pt.Result
    pt.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    assert np.array_equal(bits(pt.Result), bits(before)) and np.array_equal(bits(before), bits(acc[2]))  # image and frame counter untouched
    assert_same_image(pt.Present(), host.rgba8(acc[2]), "REFERENCE present of 3 frames")
    # the integrator is still in contract arithmetic: the next frame is the contract oracle's
    pt.Render()
    assert np.array_equal(bits(pt.Result), bits(acc[3]))
    # ... and so is the atmosphere precompute
    ubo, lp = pkg.camera.atmospheric_data_ubo(), np.asarray(pkg.camera.atmosphere_light_pos(0.4), np.float32)
    side = pkg.PathTracer(None, 16, 16, 1, 1, 1.0, 0.0)
    side.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    at = pkg.AtmosphericScatterer(16, ubo, lp, side)
    at.ISteps, at.JSteps = 8, 3
    side.EnvironmentMap = at
    assert np.array_equal(bits(at.Result), bits(oracle.atmosphere(16, ubo, lp, 15.0, 8, 3)))
    # setting the two other switches leaves the present mode alone, in either state
    assert native_lib.pt_atmosphere_set_arithmetic(side._h, N.PT_ARITH_REFERENCE) == N.PT_OK
    side.SetArithmetic(N.PT_ARITH_REFERENCE)
    img = probe.witness_tile()
    small = loaded(pkg, img)
    small.SetArithmetic(N.PT_ARITH_REFERENCE)
    assert native_lib.pt_atmosphere_set_arithmetic(small._h, N.PT_ARITH_REFERENCE) == N.PT_OK
    assert_same_image(small.Present(), oracle.postprocess(img)[1], "present mode CONTRACT with both other switches on REFERENCE")
    small.SetPresentArithmetic(N.PT_ARITH_REFERENCE)
    small.SetArithmetic(N.PT_ARITH_CONTRACT)
    assert native_lib.pt_atmosphere_set_arithmetic(small._h, N.PT_ARITH_CONTRACT) == N.PT_OK
    assert_same_image(small.Present(), host.rgba8(img), "present mode REFERENCE with both other switches back on CONTRACT")
    # a bad mode is refused and the mode in force stays
    for bad in (2, -1):
        assert native_lib.pt_present_set_arithmetic(small._h, bad) == N.PT_E_BAD_ARGUMENT
    assert_same_image(small.Present(), host.rgba8(img), "after rejected modes: still REFERENCE")
    small.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    for bad in (2, -1):
        assert native_lib.pt_present_set_arithmetic(small._h, bad) == N.PT_E_BAD_ARGUMENT
    assert_same_image(small.Present(), oracle.postprocess(img)[1], "after rejected modes: still CONTRACT")
    small.Dispose()
    side.Dispose()
    # switching with frames pending: they are launched, the accumulation is what it would have been
    pt.SetFrameBatch(0)
    for _ in range(4):
        pt.Render()
    pt.SetPresentArithmetic(N.PT_ARITH_CONTRACT)
    assert np.array_equal(bits(pt.Result), bits(acc[7]))
    assert_same_image(pt.Present(), oracle.postprocess(acc[7])[1], "CONTRACT present of 8 frames")
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ (6) cost (recorded, not gated)
def test_cost_at_1080p_is_recorded(pkg, native_lib, host, parity_report):
    """1080p pt_postprocess_device under pt_timer_*, fastest of three, both modes on one handle.  The times are recorded, not gated: they
    go into the terminal summary as the label of a parity row (tests/conftest.py's table), whose figures are the agreement of the timed
    REFERENCE pass with the host over the whole 1080p image."""
    N = pkg.native
    img = log_uniform(1080, 1920, 3)
    pt = loaded(pkg, img)
    ms = {}
    for name, mode in (("contract", N.PT_ARITH_CONTRACT), ("reference", N.PT_ARITH_REFERENCE)):
        pt.SetPresentArithmetic(mode)
        pt.PostProcessDevice()  # (first launch of the kernel: module load)
        pt.Synchronize()
        best = []
        for _ in range(3):
            pt.TimerBegin()
            pt.PostProcessDevice()
            best.append(pt.TimerEnd())
        ms[name] = min(best)
    got = pt.Present()  # (still REFERENCE)
    pt.Dispose()
    same = float((got == host.rgba8(img)).all(-1).mean())
    line = (f"tone map 1080p: contract {1000 * ms['contract']:.1f} us, reference {1000 * ms['reference']:.1f} us "
            f"({ms['reference'] / ms['contract']:.2f}x)")
    print("\n  " + line)
    parity_report(line, {"within": same, "bit_identical": same, "mean_rel_err": 0.0, "mean_abs_err": 0.0}, 1.0)
    assert same == 1.0
    assert all(0.0 < v < 1000.0 for v in ms.values())
