"""Constructed images and key lines for BinaryDescriptor::compute (LBD; Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:524-687), shared by
test_lbd_cpu.py and test_lbd_gpu.py.  Nothing here touches a device.

LBD reads four things of a key line: sPointInOctaveX/Y and ePointInOctaveX/Y (only their midpoint), numOfPixels (cast to short: the length of the
63-row support region) and angle (its direction).  Nothing ties the three together, so a scene sets them apart where that reaches code that the
detector's own key lines never reach; the other fields are filled in consistently (octave 0) and are not read.

  image(kind, W, H)        one of IMAGE_KINDS at one of SIZES
  scene(seed, W, H)        (key lines, kind index of every row): every kind of KINDS is drawn
  shifted(kls, dx, dy)     the same key lines moved by whole pixels
  flat_side(kls)           the transposed-load predicate fabsf(dL0) >= fabsf(dL1) of every row, from the float angle
  short_len(kls)           (short)numOfPixels of every row
  poison(n)                far key lines for the records past an image's count in a batch call
  slanted_checker(W, H)    an image on which LSD detects lines (for the fused entry)

The 64 x 203 image is portrait: its context describes caller-supplied key lines but runs no detector (include/orbline.h, olf_ctx_create).
"""
import numpy as np
from orb_line_slam_amd._lib import KEYLINE_DTYPE

SIZES = ((64, 64), (97, 71), (131, 64), (64, 203))            # (W, H); 64 x 64 is the smallest context
IMAGE_KINDS = ("noise", "sinusoids", "ramp", "steps", "flat")
KINDS = ("interior", "axis", "diagonal", "flat_predicate", "bad_num", "outside", "far", "angles")
SEEDS = (11, 12)
AXIS_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
BAD_NUMS = (200, 64, 65, 0, -3, 40000, 70000)                 # on a 10-pixel line; as short: 200, 64, 65, 0, -3, -25536, 4464
F32 = np.float32
PI, HPI, QPI = F32(np.pi), F32(np.pi / 2), F32(np.pi / 4)
# floats at which glibc's cosf is not the rounded double cos (found by a random search): convention C.6 changes the direction vector itself there
COSF_ANGLES = (F32(-4.4600019454956055), F32(19.830171585083008), F32(-38.57712936401367), F32(48.23119354248047), F32(68.32939910888672))


def _next(x, towards):
    return np.nextafter(F32(x), F32(towards), dtype=np.float32)


def image(kind, W, H, seed=0):
    """(H, W) uint8"""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return np.random.default_rng(1000 + seed).integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "sinusoids":
        rng = np.random.default_rng(2000 + seed)
        acc = np.zeros((H, W))
        for _ in range(12):
            fx, fy, ph, a = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1.0)
            acc += a * np.sin(fx * x + fy * y + ph)
        acc -= acc.min()
        return np.rint(acc * (255.0 / acc.max())).astype(np.uint8)
    if kind == "ramp":
        return np.clip(2 * x + y, 0, 255).astype(np.uint8)
    if kind == "steps":
        return np.where(((x // 5 + y // 7) & 1) == 1, 200, 40).astype(np.uint8)
    if kind == "flat":
        return np.full((H, W), 93, np.uint8)
    raise ValueError(kind)


def slanted_checker(W, H):
    """a two-level checker of slanted cells: LSD detects dozens of short lines on it at every one of SIZES (the fused-entry test needs detections)"""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((((x + y // 2) // 17 + (y - x // 3) // 13) & 1) == 1, 190, 60).astype(np.uint8)


def keylines(rows):
    """KEYLINE_DTYPE records from rows of (sx, sy, ex, ey, angle or None, numOfPixels or None): angle defaults to atan2 of the end points and numOfPixels
    to cv::LineIterator's count between the rounded end points, as LSDDetectorC::detectImpl fills them in"""
    k = np.zeros(len(rows), KEYLINE_DTYPE)
    for i, (sx, sy, ex, ey, ang, num) in enumerate(rows):
        sx, sy, ex, ey = F32(sx), F32(sy), F32(ex), F32(ey)
        r = k[i]
        r["startPointX"], r["startPointY"], r["endPointX"], r["endPointY"] = sx, sy, ex, ey
        r["sPointInOctaveX"], r["sPointInOctaveY"], r["ePointInOctaveX"], r["ePointInOctaveY"] = sx, sy, ex, ey
        r["pt_x"], r["pt_y"] = (sx + ex) / F32(2), (sy + ey) / F32(2)
        dx, dy = float(ex) - float(sx), float(ey) - float(sy)
        r["angle"] = F32(np.arctan2(dy, dx)) if ang is None else F32(ang)
        r["lineLength"] = F32(np.hypot(dx, dy))
        r["size"] = F32(abs(dx * dy))
        r["response"] = r["lineLength"] / F32(256)
        r["class_id"], r["octave"] = i, 0
        r["numOfPixels"] = int(max(abs(np.rint(ex) - np.rint(sx)), abs(np.rint(ey) - np.rint(sy))) + 1) if num is None else int(num)
    return k


def _around(mx, my, ang, n):
    """end points of an n-pixel line through (mx, my) along ang"""
    hx, hy = 0.5 * (n - 1) * np.cos(float(ang)), 0.5 * (n - 1) * np.sin(float(ang))
    return mx - hx, my - hy, mx + hx, my + hy


def scene(seed, W, H):
    """(kls, kind): kind[i] indexes KINDS.  About 170 key lines."""
    rng = np.random.default_rng(seed)
    rows, kind = [], []

    def add(name, *r):
        rows.append(r)
        kind.append(KINDS.index(name))

    # random lines inside the image
    for _ in range(56):
        while True:
            sx, ex = rng.uniform(0, W - 1, 2)
            sy, ey = rng.uniform(0, H - 1, 2)
            if np.hypot(ex - sx, ey - sy) >= 2:
                break
        add("interior", sx, sy, ex, ey, None, None)
    # axis-aligned lines with integer end points, both directions, on rows / columns 0, 1, mid and last: an even length has a half-integer midpoint and
    # every sample of every row of its support region is then an exact k + 0.5 tie (negative ones on row / column 0)
    j = int(rng.integers(0, 4))
    for li, L in enumerate(AXIS_LENGTHS):
        for d in range(4):                                       # 0: angle 0, 1: float(pi), 2: pi/2, 3: -pi/2
            horiz = d < 2
            span, across = (W, H) if horiz else (H, W)
            c = (0, 1, across // 2, across - 1)[(j + li + d) % 4]      # (every direction meets every position as the lengths go by)
            a0 = int(rng.integers(0, span - L + 1))
            a1 = a0 + L - 1
            if d in (1, 3):
                a0, a1 = a1, a0
            ang = (F32(0), PI, HPI, -HPI)[d]
            if horiz:
                add("axis", a0, c, a1, c, ang, L)
            else:
                add("axis", c, a0, c, a1, ang, L)
    # the two full diagonals, the four full border lines, one-pixel lines in two opposite corners
    for s in ((0, 0, W - 1, H - 1), (W - 1, 0, 0, H - 1), (0, 0, W - 1, 0), (W - 1, 0, W - 1, H - 1), (W - 1, H - 1, 0, H - 1), (0, H - 1, 0, 0)):
        add("diagonal", *s, None, None)
    add("diagonal", 0, 0, 0, 0, F32(0), 1)
    add("diagonal", W - 1, H - 1, W - 1, H - 1, PI, 1)
    # the transposed-load predicate |cos| >= |sin| flips at the four diagonals: each, and one float either side
    for base in (QPI, -QPI, F32(3) * QPI, F32(-3) * QPI):
        for ang in (_next(base, -10), base, _next(base, 10)):
            n = int(rng.integers(18, 34))
            mx, my = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H)
            add("flat_predicate", *_around(mx, my, ang, n), ang, n)
    # numOfPixels that disagrees with the end points of a 10-pixel line: longer (the rows walk out of the image), and values whose (short) is <= 0
    for num in BAD_NUMS:
        ang = rng.uniform(-np.pi, np.pi)
        mx, my = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H)
        add("bad_num", *_around(mx, my, ang, 10), None, num)
    # partly or wholly outside: end points at (-0.5, -0.5) (negative ties on the top / left border), lines 300 pixels beyond each side
    add("outside", -0.5, -0.5, W // 2 + 0.5, -0.5, F32(0), W // 2 + 2)
    add("outside", -0.5, -0.5, -0.5, H // 2 + 0.5, HPI, H // 2 + 2)
    add("outside", -0.5, -0.5, 15.5, 15.5, None, None)
    for mx, my in ((-300, H / 2), (W + 300, H / 2), (W / 2, -300), (W / 2, H + 300)):
        ang, n = rng.uniform(-np.pi, np.pi), int(rng.integers(12, 30))
        add("outside", *_around(mx + rng.uniform(-3, 3), my + rng.uniform(-3, 3), ang, n), None, n)
    # far: sample coordinates beyond +-32767, where the reference's (short) cast wraps before the clamp.  x = 40000 lands on column 0, x = -40000 on the
    # last column, y = 33000 on row 0, x = 65536 + 10 on column 10, and a horizontal line through x = 32767 straddles the cast's edge
    for mx, my, ang in ((40000, H / 2, None), (-40000, H / 2, None), (W / 2, 33000, None), (65536 + 10, H / 2, None), (65536 + 10, H / 2, 0.0),
                        (32767, H / 2, 0.0), (32767.5, H / 3, 0.3), (40000, H / 3, HPI)):
        ang = rng.uniform(-np.pi, np.pi) if ang is None else ang
        n = int(rng.integers(16, 34))
        add("far", *_around(mx, my + rng.uniform(-2, 2), ang, n), ang, n)
    # caller angles: beyond [-pi, pi] (below 120 in magnitude), exactly at +-pi and +-pi/2, and where glibc's sinf / cosf branch (2^-12, pi/4)
    tp = F32(2 * np.pi)
    for ang in (tp, -tp, _next(tp, 10), _next(tp, 0), _next(-tp, -10), _next(-tp, 0), F32(7), F32(100), F32(-100), PI, -PI, HPI, -HPI,
                F32(2.0 ** -12), _next(2.0 ** -12, 0), F32(2.0 ** -13), F32(-2.0 ** -12), F32(0), QPI, _next(QPI, 0), _next(QPI, 1), F32(3), F32(-3), F32(119.5)) + COSF_ANGLES:
        n = int(rng.integers(10, 31))
        mx, my = rng.uniform(0.25 * W, 0.75 * W), rng.uniform(0.25 * H, 0.75 * H)
        add("angles", *_around(mx, my, ang, n), ang, n)
    return keylines(rows), np.array(kind, np.int32)


def shifted(kls, dx, dy=0):
    k = kls.copy()
    for f in ("startPointX", "endPointX", "sPointInOctaveX", "ePointInOctaveX", "pt_x"):
        k[f] = k[f] + F32(dx)
    for f in ("startPointY", "endPointY", "sPointInOctaveY", "ePointInOctaveY", "pt_y"):
        k[f] = k[f] + F32(dy)
    return k


def short_len(kls):
    return kls["numOfPixels"].astype(np.int16)


def flat_side(kls):
    """fabsf(dL0) >= fabsf(dL1) with dL = (float)cos / sin((double)angle): the rows k_lbd_rows loads through its transposed LDS tile"""
    a = kls["angle"].astype(np.float64)
    return np.abs(np.cos(a).astype(np.float32)) >= np.abs(np.sin(a).astype(np.float32))


def poison(n):
    """n valid but far key lines: what a batch call keeps past an image's count"""
    return keylines([_around(40000 + 7 * i, 33000 - 5 * i, 0.4, 25) + (0.4, 25) for i in range(n)])
