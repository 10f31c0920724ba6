"""Constructed inputs for Frame::ComputeStereoMatches (src/Frame.cc:702-876): key points, descriptors and image patches placed so that every gate of
the function is hit on its boundary.  Shared by tests/test_stereo_points_cpu.py and tests/test_stereo_points_gpu.py; seeded, nothing is drawn at import.

One stereo pair cannot hold every kind -- the median filter (:862-875) works on all accepted points of a pair, so SADs near 55000 and SADs placed within
1 of 2.1 * median need pairs of their own.  The scenes therefore are
    main / main_odd   kinds clean, tie, threshold, octave, band, u_range, border, edge_shift, zero_disp, half   (320x240 / 333x257)
    saturated         kind saturated (plus a few clean points)
    median_1 / median_odd / median_even     kind median
and scene_kinds(scene) says which kind every left key point is.  A key point's `expect` entry names the branch it was built to take; the CPU tests count
them on the restatement (tests/stereo_points_reference.py), never on the GPU's output.

Layout of an image: rows 17..123 hold painted blocks (random 11x31 textures copied into both images, so the SAD at the true shift is exactly the amount
added to the left patch, and every other shift is in the thousands); rows 124.. hold a smooth texture whose right image is the left one shifted by a
per-band disparity plus +-2 noise (so ordinary points have an interior SAD minimum and a SAD above 0).

Safety: every constructed key point lies where the extractor could have put it -- round(x * inv_scale) in [16, w_l - 17] at its own level, the same for
y -- except the border kind, whose right points are rejected by endu before a pixel is read or end 1 pixel inside.  Every scene is run through the restatement as it is built
(_Builder.scene), which raises if any window or strip would leave its level image, or if a right point passes a left point's gates with scaleduR0 < 10.
"""
import functools
import numpy as np
import oracle_lib as oracle
import stereo_points_reference as ref

f32 = np.float32
W, H = 320, 240
NFEATURES, FX, BF = 500, 60.0, 6.0
PAINT_ROWS = [22 + 12 * i for i in range(9)]           # centre rows of the painted blocks (rows 17..123)
TEX_TOP = 124                                          # first row of the shifted-texture region
BANDS = [(0, 8), (124, 14), (164, 4), (200, 6)]        # (first row, disparity) of the right image's bands
KINDS = ("clean", "tie", "threshold", "octave", "band", "u_range", "border", "edge_shift", "zero_disp", "saturated", "half", "median")
SHAPES = [(0, 50), (50, 0), (1, 1), (255, 257), (256, 129), (257, 300)]


@functools.lru_cache(None)
def params():
    return oracle.full_params(NFEATURES, 100, FX, BF)


@functools.lru_cache(None)
def tables():
    sf, inv = oracle.orb_tables(params().orb)[:2]
    return sf, inv


def capacity():
    """olf_orb_capacity of a context with these parameters (the GPU test checks it against the context)"""
    return NFEATURES + 64


def max_disparity():
    """maxD as the code computes it, in float32: mb = bf / fx; maxD = bf / mb (src/Frame.cc:197, :732-734)"""
    mb = f32(BF) / f32(FX)
    return f32(BF) / mb


def band_disparity(y):
    d = BANDS[0][1]
    for top, dd in BANDS:
        if y >= top:
            d = dd
    return d


def _smooth(rng, h, w):
    a = rng.random((h + 8, w + 8))
    for _ in range(2):                                  # two passes of a 5-tap box in each direction
        a = sum(np.roll(a, s, 0) for s in range(-2, 3)) / 5
        a = sum(np.roll(a, s, 1) for s in range(-2, 3)) / 5
    a = a[4:-4, 4:-4]
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(20 + 215 * a, 0, 255).astype(np.uint8)


def _flip_bits(rng, d, k):
    out = d.copy()
    for b in rng.choice(256, k, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


class _Builder:
    def __init__(self, seed, w=W, h=H):
        self.rng = np.random.default_rng(seed)
        self.w, self.h = w, h
        self.lw, self.lh = oracle.orb_level_sizes(params().orb, w, h)
        self.sf, self.inv = tables()
        wide = _smooth(self.rng, h, w + 64)
        self.imgL = wide[:, :w].copy()
        self.imgR = np.zeros((h, w), np.uint8)
        for y in range(h):
            d = band_disparity(y)
            self.imgR[y] = wide[y, d:d + w]
        noise = self.rng.integers(-2, 3, (h, w))
        self.imgR = np.clip(self.imgR.astype(np.int32) + noise, 0, 255).astype(np.uint8)
        self.kL, self.dL, self.kR, self.dR = [], [], [], []
        self.kinds, self.expect = [], []
        self.border_pts = {"L": set(), "R": set()}      # the key points allowed past the extractor's 16-pixel margin
        self.slot_row, self.slot_x = 0, 6

    # -- key points ----------------------------------------------------------------------------------------------------------------------------------
    def in_range(self, x, y, o, border_ok=False):
        xi, yi = float(ref.c_round(f32(f32(x) * self.inv[o]))), float(ref.c_round(f32(f32(y) * self.inv[o])))
        okx = 16 <= xi <= self.lw[o] - 17 or border_ok
        return okx and 16 <= yi <= self.lh[o] - 17

    def left(self, x, y, o, desc, kind, expect, border_ok=False):
        assert 0 <= o < len(self.sf) and self.in_range(x, y, o, border_ok), (x, y, o, kind)
        if border_ok:
            self.border_pts["L"].add(len(self.kL))
        self.kL.append((f32(x), f32(y), f32(31 * self.sf[o]), f32(0), f32(20), o, -1))
        self.dL.append(desc)
        self.kinds.append(kind)
        self.expect.append(expect)
        return len(self.kL) - 1

    def right(self, x, y, o, desc, border_ok=False):
        assert 0 <= o < len(self.sf) and self.in_range(x, y, o, border_ok), (x, y, o)
        if border_ok:
            self.border_pts["R"].add(len(self.kR))
        self.kR.append((f32(x), f32(y), f32(31 * self.sf[o]), f32(0), f32(20), o, -1))
        self.dR.append(desc)
        return len(self.kR) - 1

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, d, k):
        return _flip_bits(self.rng, d, k)

    def tex_pos(self, o, rows=None, need=62):
        """a level-o grid position in the texture region, as the extractor reports it (pt * scale, float32); `need` level-0 pixels are free to its left"""
        lo, hi = rows or (TEX_TOP + 4, self.h - 21)
        s = float(self.sf[o])
        ylo, yhi = max(16, int(np.ceil(lo / s))), min(int(self.lh[o]) - 17, int(np.floor(hi / s)))
        xlo, xhi = 16 + int(np.ceil((need + 2) / s)), int(self.lw[o]) - 17
        assert ylo <= yhi and xlo <= xhi, o
        xi, yi = int(self.rng.integers(xlo, xhi + 1)), int(self.rng.integers(ylo, yhi + 1))
        return f32(f32(xi) * self.sf[o]), f32(f32(yi) * self.sf[o])

    # -- painted blocks ------------------------------------------------------------------------------------------------------------------------------
    def slot(self, d):
        """(xL, y) of a painted feature of disparity d whose 31-wide blocks in both images overlap nobody else's"""
        if self.slot_x + 15 + d + 15 > self.w - 1 or self.slot_x + 15 + d > self.w - 17:
            self.slot_row, self.slot_x = self.slot_row + 1, 6
        assert self.slot_row < len(PAINT_ROWS), "painted region is full"
        xR = self.slot_x + 15
        self.slot_x = xR + d + 17
        return xR + d, PAINT_ROWS[self.slot_row]

    def paint(self, xL, y, xR, sad=0, symmetric=False, T=None):
        """the same 11x31 texture around (xL, y) in the left and (xR, y) in the right image; the left 11x11 patch gets `sad` added (mirror-symmetric, centre
        untouched), so SAD(true shift) == sad exactly"""
        if T is None:
            T = self.rng.integers(40, 216, (11, 31))
            if symmetric:
                T[:, 16:] = T[:, 14::-1]
        for img, cx in ((self.imgL, xL), (self.imgR, xR)):
            for c in range(31):
                x = cx - 15 + c
                if 0 <= x < self.w:
                    img[y - 5:y + 6, x] = T[:, c]
        e = np.zeros((11, 11), np.int64)
        left = sad
        if left & 1:
            e[0, 5] += 1
            left -= 1
        for r in range(11):
            for c in range(5):
                q = min(20, left // 2)
                e[r, c] += q
                e[r, 10 - c] += q
                left -= 2 * q
        assert left == 0 and e[5, 5] == 0
        self.imgL[y - 5:y + 6, xL - 5:xL + 6] = (self.imgL[y - 5:y + 6, xL - 5:xL + 6].astype(np.int64) + e).astype(np.uint8)
        return T

    def painted_pair(self, d, shift, kind, expect, sad=None, symmetric=False, k=20, T=None, xr_kp=None):
        """a painted feature whose true right position is xL - d and whose right key point sits `shift` pixels left of it (the SAD minimum is at +shift)"""
        xL, y = self.slot(d)
        T = self.paint(xL, y, xL - d, int(self.rng.integers(60, 240)) if sad is None else sad, symmetric, T)
        dl = self.desc()
        iR = self.right(xL - d - shift if xr_kp is None else xr_kp(xL), y, 0, self.flipped(dl, k))
        expect = dict(expect)
        if expect.pop("own", True):
            expect["iR"] = iR
        iL = self.left(xL, y, 0, dl, kind, expect)
        return iL, iR, T

    # -- the kinds -----------------------------------------------------------------------------------------------------------------------------------
    def clean(self, n, kind="clean"):
        for _ in range(n):
            o = int(self.rng.integers(0, len(self.sf)))
            x, y = self.tex_pos(o)
            d = band_disparity(int(y))
            dl = self.desc()
            iR = self.right(f32(x - f32(d)), y, o, self.flipped(dl, int(self.rng.integers(0, 50))))
            self.left(x, y, o, dl, kind, dict(iR=iR, reached="sad"))

    def tie(self):
        for i in range(8):
            o = i % 2
            x, y = self.tex_pos(o, need=84)
            d = band_disparity(int(y))
            dl = self.desc()
            true_pt, false_pt = f32(x - f32(d)), f32(x - f32(d) - f32(20))
            first_row, second_row = (f32(y - 1), f32(y + 1)) if i < 4 else (f32(y + 1), f32(y - 1))   # index order along / against row order
            first_x, second_x = (true_pt, false_pt) if (i >> 1) % 2 == 0 else (false_pt, true_pt)
            a = self.right(first_x, first_row, o, self.flipped(dl, 30))
            b = self.right(second_x, second_row, o, self.flipped(dl, 30))
            assert a < b
            self.left(x, y, o, dl, "tie", dict(iR=a, bestDist=30))

    def threshold(self):
        for i, k in enumerate([74, 75, 99, 100] * 2):
            x, y = self.tex_pos(0)
            d = band_disparity(int(y))
            dl = self.desc()
            iR = self.right(f32(x - f32(d)), y, 0, self.flipped(dl, k))
            e = dict(iR=iR, bestDist=74, reached="sad") if k == 74 else dict(bestDist=k, tag="no_match")
            if k == 99:
                e["iR"] = iR
            self.left(x, y, 0, dl, "threshold", e)

    def octave(self):
        for i in range(8):
            lv, s = 2 + i % 4, (1 if i < 4 else -1)
            x, y = self.tex_pos(lv, rows=(TEX_TOP + 4, 176), need=84)      # (rows that exist on level 7 too)
            d = band_disparity(int(y))
            dl = self.desc()
            self.right(f32(x - f32(d) - f32(20)), y, lv + 2 * s, self.flipped(dl, 10))      # nearest descriptor, two octaves away: must not be seen
            far = self.right(f32(x - f32(d)), y, lv + s, self.flipped(dl, 40))
            self.left(x, y, lv, dl, "octave", dict(iR=far, bestDist=40, reached="sad"))

    def band(self):
        for o in (0, 7):
            for case in ("minr", "maxr", "minr-1", "maxr+1"):
                x, y = self.tex_pos(o, rows=(TEX_TOP + 12, 166))
                d = band_disparity(int(y))
                yr = f32(np.floor(y) + f32(0.37))
                r = f32(2.0) * self.sf[o]
                minr, maxr = int(np.floor(f32(yr - r))), int(np.ceil(f32(yr + r)))
                row = dict(minr=minr, maxr=maxr)
                row.update({"minr-1": minr - 1, "maxr+1": maxr + 1})
                yl = f32(row[case] + (0.25 if o else 0.0))
                dl = self.desc()
                iR = self.right(f32(x - f32(band_disparity(int(yl)))), yr, o, self.flipped(dl, 25))
                inside = case in ("minr", "maxr")
                self.left(x, yl, o, dl, "band", dict(iR=iR, bestDist=25) if inside else dict(not_iR=iR, tag_in=("no_match", "no_row_cand")))

    def u_range(self):
        maxD = max_disparity()
        for rep in range(2):
            for case in ("minU", "below", "maxU", "above"):
                if case in ("minU", "below"):
                    # the painted copy sits 59 pixels to the left; the key point on (or one ulp below) uL - maxD, one more pixel to the left
                    fn = (lambda xL: f32(f32(xL) - maxD)) if case == "minU" else (lambda xL: np.nextafter(f32(f32(xL) - maxD), f32(-np.inf)))
                    d = int(maxD) - 1
                else:
                    fn = (lambda xL: f32(xL)) if case == "maxU" else (lambda xL: np.nextafter(f32(xL), f32(np.inf)))
                    d = 0
                e = dict(reached="sad", tag="ok") if case in ("minU", "maxU") else dict(own=False, tag="no_match", bestDist=ref.TH_HIGH)
                self.painted_pair(d, 0, "u_range", e, symmetric=True, xr_kp=fn)

    def border(self):
        w0 = self.w
        for rep in range(2):
            for keep in (True, False):
                # level 0: endu = scaleduR0 + 11 is w - 1 (kept) or w (rejected); left and right 4 pixels apart, in the band of disparity 4
                y = f32(170 + 9 * rep + (4 if keep else 0))
                xr = w0 - 12 if keep else w0 - 11
                dl = self.desc()
                iR = self.right(f32(xr), y, 0, self.flipped(dl, 20), border_ok=True)
                self.left(f32(xr + 4), y, 0, dl, "border", dict(iR=iR, reached="sad") if keep else dict(iR=iR, tag="endu"), border_ok=True)
                # level 2, in the band of disparity 6 (4 level pixels)
                lv = 2
                wl = int(self.lw[lv])
                xi = wl - 12 if keep else wl - 11
                yi = int(np.ceil(204 / float(self.sf[lv]))) + 5 * rep + (2 if keep else 0)
                xrf, xlf, yf = f32(f32(xi) * self.sf[lv]), f32(f32(xi + 4) * self.sf[lv]), f32(f32(yi) * self.sf[lv])
                assert ref.c_round(f32(xrf * self.inv[lv])) == xi and xlf <= w0 - 1
                dl = self.desc()
                iR = self.right(xrf, yf, lv, self.flipped(dl, 20), border_ok=True)
                self.left(xlf, yf, lv, dl, "border", dict(iR=iR, reached="sad") if keep else dict(iR=iR, tag="endu"), border_ok=True)

    def edge_shift(self):
        for rep in range(2):
            for s in (-5, -4, 4, 5):
                e = dict(bestinc=s, tag="edge_inc") if abs(s) == 5 else dict(bestinc=s, reached="sad", tag="ok")
                self.painted_pair(8, s, "edge_shift", e)

    def zero_disp(self):
        for rep in range(4):
            self.painted_pair(0, 0, "zero_disp", dict(bestinc=0, tag="ok", zero=True), symmetric=True)
        for rep in range(4):
            # bestuR above uL by a sub-pixel deltaR: needs SAD(-1) > SAD(+1); a texture whose fit leans the other way is mirrored
            T = self.rng.integers(40, 216, (11, 31))
            L = T[:, 10:21] - T[5, 15]
            sm = np.abs(L - (T[:, 9:20] - T[5, 14])).sum()
            sp = np.abs(L - (T[:, 11:22] - T[5, 16])).sum()
            if sm <= sp:
                T = T[:, ::-1].copy()
            self.painted_pair(0, 0, "zero_disp", dict(bestinc=0, tag="disparity"), sad=0, T=T)

    def half(self):
        for lv in (0, 1):
            made = 0
            while made < 4:
                x, y = self.tex_pos(lv)
                d = band_disparity(int(y))
                m = float(ref.c_round(f32(x * self.inv[lv])))
                m -= m % 2                                             # an even m: round-half-even and round-half-away disagree on m + 0.5
                xh = self.half_x(m, lv)
                xrh = self.half_x(m - round(d / float(self.sf[lv])), lv)
                if xh is None or xrh is None:
                    continue
                dl = self.desc()
                iR = self.right(xrh, y, lv, self.flipped(dl, 20))
                self.left(xh, y, lv, dl, "half", dict(iR=iR, reached="sad", half=True))
                made += 1

    def half_x(self, m, lv):
        """a float32 x with x * inv_scale[lv] == m + 0.5 exactly (in float32), or None"""
        x = f32((m + 0.5) * float(self.sf[lv]))
        for _ in range(8):
            x = np.nextafter(x, f32(-np.inf))
        for _ in range(17):
            if f32(x * self.inv[lv]) == f32(m + 0.5):
                return x
            x = np.nextafter(x, f32(np.inf))
        return None

    def saturated(self, n):
        ramp = np.clip(60 - 6 * np.abs(np.arange(21) - 12), 0, 255)
        for _ in range(n):
            xL, y = self.slot(6)
            xR = xL - 6
            self.imgL[y - 5:y + 6, xL - 5:xL + 6] = 255
            self.imgL[y, xL] = 0
            self.imgR[y - 5:y + 6, xR - 10:xR + 11] = ramp[None, :]
            self.imgR[y, xR - 10:xR + 11] = 255
            dl = self.desc()
            iR = self.right(xR, y, 0, self.flipped(dl, 20))
            self.left(xL, y, 0, dl, "saturated", dict(iR=iR, bestinc=2, tag="ok", big=True))

    def median(self, sads, keep):
        for s, kp in zip(sads, keep):
            self.painted_pair(8, 0, "median", dict(bestinc=0, sad0=s, tag="ok" if kp else "median"), sad=s)

    # -- result --------------------------------------------------------------------------------------------------------------------------------------
    def scene(self, name, nL=None, nR=None):
        base = (len(self.kL), len(self.kR))
        while (nL is not None and len(self.kL) < nL) or (nR is not None and len(self.kR) < nR):
            self.clean(1, "clean")
        nL, nR = len(self.kL) if nL is None else nL, len(self.kR) if nR is None else nR
        kpsL = np.array(self.kL[:nL], oracle.KEYPOINT_DTYPE) if nL else np.zeros(0, oracle.KEYPOINT_DTYPE)
        kpsR = np.array(self.kR[:nR], oracle.KEYPOINT_DTYPE) if nR else np.zeros(0, oracle.KEYPOINT_DTYPE)
        descL = np.array(self.dL[:nL], np.uint8).reshape(-1, 32)
        descR = np.array(self.dR[:nR], np.uint8).reshape(-1, 32)
        whole = nL >= base[0] and nR >= base[1]        # every constructed point is in: the expectations hold
        s = dict(name=name, w=self.w, h=self.h, imgL=self.imgL, imgR=self.imgR, kpsL=kpsL, descL=descL, kpsR=kpsR, descR=descR,
                 kinds=list(self.kinds[:nL]), expect=self.expect[:nL] if whole else [{}] * nL, whole=whole, border_pts=self.border_pts)
        s["ref"] = reference(s)                        # raises SceneError if a window or strip leaves its level: the scene would be invalid
        return s


def pyramids(scene):
    p = params()
    return (oracle.orb_extract(scene["imgL"], p.orb, debug=True)["pyramid"], oracle.orb_extract(scene["imgR"], p.orb, debug=True)["pyramid"])


def reference(scene, mutate=None):
    """the restatement's answer for a scene"""
    if "pyr" not in scene:
        scene["pyr"] = pyramids(scene)
    sf, inv = tables()
    return ref.compute_stereo_matches(scene["kpsL"], scene["descL"], scene["kpsR"], scene["descR"], scene["pyr"][0], scene["pyr"][1], sf, inv, BF, FX,
                                      mutate=mutate)


def oracle_answer(scene):
    if "oracle" not in scene:
        scene["oracle"] = oracle.stereo_match_keys(scene["imgL"], scene["imgR"], params(), scene["kpsL"], scene["descL"], scene["kpsR"], scene["descR"])
    return scene["oracle"]


def scene_kinds(scene):
    return list(scene["kinds"])


def _main(seed, w, h, name, nL=None, nR=None):
    b = _Builder(seed, w, h)
    b.clean(12)
    b.tie(); b.threshold(); b.octave(); b.band(); b.u_range(); b.border(); b.edge_shift(); b.zero_disp(); b.half()
    return b.scene(name, nL, nR)


def median_threshold():
    """(M, th): a median whose threshold 1.5f * 1.4f * M is a whole number in float32, so a SAD can sit exactly on it"""
    for M in range(100, 400):
        th = f32(f32(f32(1.5) * f32(1.4)) * f32(M))
        if th == np.floor(th):
            return M, int(th)
    raise AssertionError("no whole threshold")


@functools.lru_cache(None)
def main_scene():
    return _main(11, W, H, "main")


@functools.lru_cache(None)
def kind_scenes():
    """the scenes that draw the kinds, every constructed point included"""
    out = [main_scene(), _main(12, 333, 257, "main_odd")]
    b = _Builder(13)
    b.saturated(12)
    b.clean(3)
    out.append(b.scene("saturated"))
    M, th = median_threshold()
    for name, sads, keep in (("median_1", [50], [True]),
                             ("median_odd", [30, 31, 32, M, th - 1, th, th + 1], [True] * 5 + [False] * 2),
                             ("median_even", [30, 31, 32, 40, M, th - 1, th, th + 1], [True] * 6 + [False] * 2)):
        b = _Builder(20 + len(sads))
        b.median(sads, keep)
        out.append(b.scene(name))
    return out


@functools.lru_cache(None)
def shape_scenes():
    """the main scene cut or filled to the (nL, nR) shapes: 256 left points per candidate block, 128 right points per tile, 4 left points per match block"""
    out = [_main(30 + i, W, H, f"shape_{nL}x{nR}", nL, nR) for i, (nL, nR) in enumerate(SHAPES)]
    cap = capacity()
    out.append(_main(40, W, H, f"shape_{cap}x{cap}", cap, cap))
    return out


def full_scene():
    return shape_scenes()[-1]


def all_scenes():
    return kind_scenes() + shape_scenes()


# ---- scenes whose answers are derived by hand ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def hand_scenes():
    """(scene, uRight, depth) with the expected arrays written down from the construction, not computed by any implementation:
    a painted patch copied d pixels to the left and a right key point on the copy give a SAD minimum at shift 0; with a mirror-symmetric texture the two
    neighbours are equal, deltaR = 0 and bestuR = uR0 exactly, so uRight = uL - d and depth = bf / d in float32."""
    out = []
    bf = f32(BF)

    def done(b, name, ur, dp):
        s = b.scene(name)
        out.append((s, np.array(ur, f32), np.array(dp, f32)))

    # 1. a symmetric patch shifted by d = 7, 23 and 41
    b = _Builder(101)
    ur, dp = [], []
    for d in (7, 23, 41):
        iL, _, _ = b.painted_pair(d, 0, "clean", {}, sad=40, symmetric=True)
        ur.append(f32(b.kL[iL][0] - f32(d))); dp.append(bf / f32(d))
    done(b, "hand_shift", ur, dp)
    # 2. best descriptor distance 74 is matched, 75 is not (thOrbDist = 75, strict)
    b = _Builder(102)
    ur, dp = [], []
    for k in (74, 75):
        iL, _, _ = b.painted_pair(9, 0, "threshold", {}, sad=40, symmetric=True, k=k)
        ur.append(f32(b.kL[iL][0] - f32(9)) if k == 74 else f32(-1)); dp.append(bf / f32(9) if k == 74 else f32(-1))
    done(b, "hand_threshold", ur, dp)
    # 3. a tie: two right points at distance 30, the patch copied under both (12 and 45 pixels to the left); the lower INDEX wins, whichever row it is on
    b = _Builder(103)
    ur, dp = [], []
    for first, second, rows in ((12, 45, (-1, 1)), (45, 12, (-1, 1)), (12, 45, (1, -1)), (45, 12, (1, -1))):
        xL, y = b.slot(46)
        T = b.paint(xL, y, xL - 45, 0, True)
        b.paint(xL, y, xL - 12, 40, True, T)
        dl = b.desc()
        b.right(xL - first, y + rows[0], 0, b.flipped(dl, 30))
        b.right(xL - second, y + rows[1], 0, b.flipped(dl, 30))
        b.left(xL, y, 0, dl, "tie", {})
        ur.append(f32(xL - first)); dp.append(bf / f32(first))
    done(b, "hand_tie", ur, dp)
    # 4. the right border: scaleduR0 + 11 == w - 1 is searched, == w is rejected (endu >= cols)
    b = _Builder(104)
    ur, dp = [], []
    for i, xr in enumerate((W - 12, W - 11)):
        y = PAINT_ROWS[2 * i]
        b.paint(xr + 4, y, xr, 40, True)
        dl = b.desc()
        b.right(xr, y, 0, b.flipped(dl, 20), border_ok=True)
        b.left(xr + 4, y, 0, dl, "border", {}, border_ok=True)
        ur.append(f32(xr) if i == 0 else f32(-1)); dp.append(bf / f32(4) if i == 0 else f32(-1))
    done(b, "hand_border", ur, dp)
    # 5. zero disparity: bestuR == uL, so disparity = 0.01f and bestuR = (float)((double)uL - 0.01)
    b = _Builder(105)
    iL, _, _ = b.painted_pair(0, 0, "zero_disp", {}, sad=40, symmetric=True)
    done(b, "hand_zero", [f32(float(b.kL[iL][0]) - 0.01)], [bf / f32(0.01)])
    # 6. the median filter: SADs 100, 100, 300 -> median 100 (element 3 / 2 = 1), threshold 210: the third match is dropped
    b = _Builder(106)
    ur, dp = [], []
    for s in (100, 100, 300):
        iL, _, _ = b.painted_pair(5, 0, "median", {}, sad=s, symmetric=True)
        ur.append(f32(b.kL[iL][0] - f32(5)) if s < 210 else f32(-1)); dp.append(bf / f32(5) if s < 210 else f32(-1))
    done(b, "hand_median", ur, dp)
    return out


# ---- a context-filling scene for the capacity edge of the two LDS sorts ----------------------------------------------------------------------------------
def big_scene(w, h, n, seed=77, per_row=64):
    """n left and n right level-0 key points on a w x h shifted texture (disparity 9), `per_row` of them on every used row: the row sort and the median
    sort get a full array, the candidate search long rows, and the median filter has matches to drop.  Returns (imgL, imgR, kpsL, descL, kpsR, descR)."""
    rng = np.random.default_rng(seed)
    wide = _smooth(rng, h, w + 16)
    imgL, imgR = wide[:, :w].copy(), wide[:, 9:9 + w].copy()
    rows = (n + per_row - 1) // per_row
    noise = rng.integers(-2, 3, (h, w))
    noisy_from = 20 + (4 * rows // 5) * ((h - 40) // rows)          # the lowest fifth of the used rows: SADs several times the median, the filter drops them
    noise[noisy_from:] = rng.integers(-12, 13, (h - noisy_from, w))
    imgR = np.clip(imgR.astype(np.int32) + noise, 0, 255).astype(np.uint8)
    assert rows <= h - 40
    kL, kR = np.zeros(n, oracle.KEYPOINT_DTYPE), np.zeros(n, oracle.KEYPOINT_DTYPE)
    i = np.arange(n)
    x = 90 + (i % per_row) * ((w - 17 - 90) // per_row) + rng.integers(0, 3, n)
    y = 20 + (i // per_row) * ((h - 40) // rows)
    order = rng.permutation(n)                          # index order unrelated to row order
    kL["x"][order], kL["y"][order] = x, y
    kR["x"][order], kR["y"][order] = x - 9, y
    for k in (kL, kR):
        k["size"], k["response"], k["class_id"] = 31, 20, -1
    descL = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    descR = descL.copy()
    flips = rng.integers(0, 256, (n, 3))                # up to 3 bits differ
    for c in range(3):
        descR[i, flips[:, c] >> 3] ^= (1 << (flips[:, c] & 7)).astype(np.uint8)
    assert x.min() - 9 - 10 >= 16 and x.max() <= w - 17 and y.min() >= 16 and y.max() <= h - 17
    return imgL, imgR, kL, descL, kR, descR


def expectation_met(scene, r, i):
    """does left key point i take, in the answer r of the restatement, the branch it was built for?"""
    e = scene["expect"][i]
    if not e:
        return None
    ok = True
    if "iR" in e:
        ok &= int(r["iR"][i]) == e["iR"] and (int(r["bestDist"][i]) < ref.TH_HIGH or e.get("tag") == "no_match")
    if "not_iR" in e:
        ok &= int(r["iR"][i]) != e["not_iR"] or int(r["bestDist"][i]) == ref.TH_HIGH
    if "bestDist" in e:
        ok &= int(r["bestDist"][i]) == e["bestDist"]
    if "tag" in e:
        ok &= str(r["tag"][i]) == e["tag"]
    if "tag_in" in e:
        ok &= str(r["tag"][i]) in e["tag_in"]
    if e.get("reached") == "sad":
        ok &= int(r["sads"][i, 0]) >= 0
    if "bestinc" in e:
        ok &= int(r["sads"][i, 0]) >= 0 and int(r["bestinc"][i]) == e["bestinc"]
    if "sad0" in e:
        ok &= int(r["sads"][i, 5]) == e["sad0"]
    if e.get("zero"):
        ok &= r["uRight"][i] == f32(float(scene["kpsL"]["x"][i]) - 0.01) and r["depth"][i] == f32(BF) / f32(0.01)
    if e.get("half"):
        lv = int(scene["kpsL"]["octave"][i])
        p = f32(scene["kpsL"]["x"][i] * tables()[1][lv])
        ok &= float(p) % 1.0 == 0.5
    if e.get("big"):
        b = int(r["bestinc"][i]) + 5
        ok &= int(r["sads"][i, b - 1:b + 2].max()) >= 32768
    return bool(ok)
