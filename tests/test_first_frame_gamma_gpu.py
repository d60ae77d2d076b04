"""GPU: the step kernels' gamma code -- pow_gamma and the frame-1 shortcut that leaves FromGamma(old)
out when a wave's stored values are all in the safe set -- against plain per-frame launches of the tile
schedule (kernel_entry: the library pow, no shortcut) in the same math mode, bit for bit; pinned also
against the CPU oracle.

The output buffer is written before every launch.  16x8 (two 8x8 tiles, one accumulation wave each; the
camera inside the box, so every pixel reaches the gamma chain): the left tile holds benign values, so
its wave takes the shortcut, the right tile holds one adversarial value in one lane, so its wave must
fall back (the denormal, -0 and 2^57 are inside the set: that wave may take the shortcut too).  64x64
with the bench camera: sky and hits mixed, one adversarial value per tile.  Runs: fused 2-frame launches
from frame 1 (shortcut at s = 0),
from frame 0 (frame number 1 arrives at s = 1 over the chain's own value) and from frame 2 (never),
single per-frame launches at frames 1 and 2 rendering into the output (perframe_defer 0) or through the
accumulation (1, and 2 = when the previous frame still runs), and the frame-0 encoding of
rtEnqueueTracePaths.  Last: the sky key and the pixels it stands for still agree through the new pow."""
import numpy as np
import pytest

from clrt import _native as N
from hip_helpers import DEFAULT_CAMERA, HipRenderer, rgb

pytestmark = pytest.mark.gpu

MATHS = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}
INSIDE = ((0.0, 1.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))   # inside the Cornell box, facing its back wall
BOUNCES = 4


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


ADVERSARIAL = {
    "nan": _f(0x7FC00001), "inf": np.float32(np.inf), "minus_one": np.float32(-1.0),
    "flt_max": np.finfo(np.float32).max, "denormal": _f(0x00000123), "minus_zero": _f(0x80000000),
    "two_pow_57": _f(0x5C000000), "above_two_pow_57": _f(0x5C000001),
}


def _benign(n, seed):
    """stored values as earlier frames leave them, with the set's corners among them"""
    rng = np.random.default_rng(seed)
    img = np.zeros((n, 4), np.float32)
    img[:, :3] = rng.random((n, 3), dtype=np.float32) * np.float32(1.5)
    img[::7, 0] = 0.0
    img[3::11, 1] = 1.0
    img[5::13, 2] = _f(0x5C000000)
    return img


def _stale_16x8(value, case):
    """left tile benign; right tile benign but for `value` in one component of one lane"""
    img = _benign(128, 1)
    lane = (7 * case + 3) % 64
    x, y = 8 + (lane & 7), lane >> 3
    img[y * 16 + x, case % 3] = value
    return img


def _stale_64x64(value):
    """one adversarial value in every 8x8 tile, lane and component moving from tile to tile"""
    img = _benign(64 * 64, 2)
    for t in range(64):
        lane = (5 * t + 1) % 64
        x, y = (t % 8) * 8 + (lane & 7), (t // 8) * 8 + (lane >> 3)
        img[y * 64 + x, t % 3] = value
    return img


class Rig:
    """one renderer per math mode and image, switched between the two schedules"""

    def __init__(self, scene, W, H, math, camera):
        self.r = HipRenderer(scene, W, H, math=math, hits=True)
        self.camera = camera
        self.r.k.set_tuning("perframe_defer_min", 0)

    def run(self, stale, first, n, sched, fused=False, defer=0):
        """the image after frames first .. first + n - 1 over `stale`, and after each frame when not fused"""
        r = self.r
        r.k.set_schedule(sched)
        r.k.set_tuning("perframe_defer", defer)
        r.ctx.WriteBuffer(r.out, stale)
        if fused:
            r.frame(first, light_bounces=BOUNCES, camera=self.camera, n_frames=n)
            return [r.result()]
        outs = []
        for f in range(first, first + n):
            r.frame(f, light_bounces=BOUNCES, camera=self.camera)
            outs.append(r.result())
        return outs

    def close(self):
        self.r.close()


@pytest.fixture(scope="module")
def rig(cornell):
    made = {}

    def get(math, W, H, camera):
        key = (math, W, H)
        if key not in made:
            made[key] = Rig(cornell, W, H, MATHS[math], camera)
        return made[key]

    yield get
    for g in made.values():
        g.close()


def _same(got, want, what):
    assert got.tobytes() == want.tobytes(), \
        f"{what}: {(got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()} pixels differ"


def _check(g, stale, tag):
    for first in (1, 0, 2):
        want = g.run(stale, first, 2, N.SCHED_TILES)
        _same(g.run(stale, first, 2, N.SCHED_STEP, fused=True)[0], want[1], f"{tag}: fused frames {first}, {first + 1}")
        if first != 0:  # the single per-frame launches at frames 1 and 2
            for defer in (0, 1, 2):
                _same(g.run(stale, first, 1, N.SCHED_STEP, defer=defer)[0], want[0],
                      f"{tag}: per-frame launch at frame {first}, perframe_defer {defer}")
    return want


@pytest.mark.parametrize("name", list(ADVERSARIAL))
@pytest.mark.parametrize("math", list(MATHS))
def test_two_tiles_one_adversarial_lane(rig, math, name):
    g = rig(math, 16, 8, INSIDE)
    case = list(ADVERSARIAL).index(name)
    stale = _stale_16x8(ADVERSARIAL[name], case)
    _check(g, stale, f"{math} {name}")
    ids, _ = g.r.hits()
    assert (ids >= 0).all()   # every pixel went through the chain: no sky shortcut


@pytest.mark.parametrize("name", ["nan", "minus_zero", "above_two_pow_57"])
@pytest.mark.parametrize("math", list(MATHS))
def test_sky_and_hits_mixed(rig, math, name):
    g = rig(math, 64, 64, DEFAULT_CAMERA)
    _check(g, _stale_64x64(ADVERSARIAL[name]), f"{math} {name} 64x64")
    ids, _ = g.r.hits()
    assert 0.1 < (ids < 0).mean() < 0.9


@pytest.mark.parametrize("W,H,camera", [(16, 8, INSIDE), (64, 64, DEFAULT_CAMERA)])
def test_pinned_equals_oracle(cornell, oracle_mod, rig, W, H, camera):
    g = rig("pinned", W, H, camera)
    stale = _stale_16x8(ADVERSARIAL["inf"], 1) if W == 16 else _stale_64x64(ADVERSARIAL["minus_one"])
    got = g.run(stale, 1, 2, N.SCHED_STEP, fused=True)[0]
    res = stale.copy()
    for f in (1, 2):
        oracle_mod.render(cornell, W, H, frame_count=f, light_bounces=BOUNCES, camera=camera, result=res, threads=16)
    assert rgb(got).tobytes() == rgb(res).tobytes()


@pytest.mark.parametrize("math", list(MATHS))
def test_trace_paths_frame0_encoding(rig, math):
    """rtEnqueueTracePaths' frame-0 encoding (the step family's gamma code) over the camera paths of frame 0
    against the tile schedule's frame 0 (the plain gamma code)"""
    g = rig(math, 64, 64, DEFAULT_CAMERA)
    n = 64 * 64
    want = g.run(np.zeros((n, 4), np.float32), 0, 1, N.SCHED_TILES)[0]
    r = g.r
    bufs = [r.ctx.create_buffer(N.MEM_READ_WRITE, n * size) for size in (N.RAY_DTYPE.itemsize, 4, 16)]
    try:
        r.k.set_uint(N.FRAME_COUNT, 0)
        r.ctx.CameraPaths(r.k, n, bufs[0], bufs[1])
        r.ctx.TracePaths(r.k, bufs[0], bufs[2], n, seeds=bufs[1], encoding=N.TRACE_FRAME0)
        res = np.empty(n, N.PATH_RESULT_DTYPE)
        r.ctx.ReadBuffer(bufs[2], res, blocking=True)
    finally:
        for b in bufs:
            b.release()
    assert np.ascontiguousarray(res["radiance"]).tobytes() == rgb(want).tobytes()


@pytest.mark.parametrize("math", list(MATHS))
def test_sky_key_agrees_with_its_pixels(rig, math):
    """Stale all-sky content, frame 1 per-frame twice: the second launch's key is the first launch's
    K_out, so its all-sky pixels take the shortcut -- and must equal the tile schedule's, computed per
    pixel with the plain pow."""
    g = rig(math, 64, 64, DEFAULT_CAMERA)
    n = 64 * 64
    sky = g.run(np.zeros((n, 4), np.float32), 0, 1, N.SCHED_TILES)[0]
    ids, _ = g.r.hits()
    miss = ids < 0
    k = sky[miss][0]
    assert miss.sum() > n // 10 and (sky[miss] == k).all()
    stale = np.tile(k, (n, 1))   # every pixel holds what an all-sky pixel holds
    r = g.r
    for defer in (0, 1):
        want = g.run(stale, 1, 1, N.SCHED_TILES)[0]
        want2 = g.run(want, 1, 1, N.SCHED_TILES)[0]
        r.k.set_schedule(N.SCHED_STEP)
        r.k.set_tuning("perframe_defer", defer)
        r.ctx.WriteBuffer(r.out, stale)
        r.frame(1, light_bounces=BOUNCES)
        first = r.result()
        r.frame(1, light_bounces=BOUNCES)
        second = r.result()
        _same(first, want, f"{math} defer {defer}: first launch")
        _same(second[miss], want2[miss], f"{math} defer {defer}: second launch, sky pixels")
        _same(second, want2, f"{math} defer {defer}: second launch")
