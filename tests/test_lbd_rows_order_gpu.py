"""GPU parity of LBD where k_lbd_rows's mapping of workgroups to (image, group of four lines) matters: batches on both sides of a multiple of eight images
(the XCD count; a mapping that keeps an image's lines on one XCD was measured and removed, profiles/README.md, and any later one has to pass here), images with
fewer lines than the capacity, an empty image inside the batch, a last group of four that is partly filled.  Both instances of the kernel are covered: the
detector's own key lines (olf_line_extract) and a caller's (olf_lbd_compute).  Every descriptor must equal the CPU oracle's.

Contexts of 1, 7, 8, 9 and 17 images at 96 x 64 and 160 x 120 with a capacity of 10 key lines (three groups of four, the last one partly filled); per image
0, 1, 3, 4, 5 or 10 lines, different from image to image, with an empty image inside the batch.

  caller's key lines    lengths 1, 15, 16, 17 and 33 (the 16-sample step and its tails), angles one float either side of |cos| = |sin| in every quadrant
                        and on the axes, centres inside the image and a few pixels beyond each of its four sides
  detector's key lines  staircase images with as many parallel edges as the image shall have lines, their direction either side of the diagonal: the
                        detector's lines run from border to border (their support regions leave the image at both ends) and it reports nothing shorter than
                        about ten pixels, so the lengths of the first list are not reached on this path; the counts are."""
import functools
import numpy as np
import pytest
import orb_line_slam_amd as ola
import lbd_scenes as S

pytestmark = pytest.mark.gpu

CAP = 10
SIZES = ((96, 64), (160, 120))
N_IMAGES = (1, 7, 8, 9, 17)
COUNT_CYCLE = (5, 0, CAP, 1, 4, 3)                               # image i holds COUNT_CYCLE[i % 6] lines: image 1 is empty, image 2 full
LENGTHS = (1, 15, 16, 17, 33)
F32 = np.float32
QPI = S.QPI
ANGLES = tuple(a for base in (QPI, -QPI, F32(3) * QPI, F32(-3) * QPI) for a in (S._next(base, -10), S._next(base, 10))) + (F32(0), S.HPI)
KINDS = ("noise", "sinusoids", "ramp", "steps")


def _count(i):
    return COUNT_CYCLE[i % len(COUNT_CYCLE)]


def _extractor(n):
    ex = ola.Lineextractor(CAP, 0.025, max_images=n)
    ex._params.orb.nlevels = 1                                   # a context needs 62 x 62 pixels on every ORB pyramid level: these images have one
    return ex


# ---- a caller's key lines ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pool(W, H):
    """every length x angle once, the centre cycling through the interior and a position 3 pixels beyond each side"""
    centres = ((W / 2, H / 2), (-3, H / 2), (W + 2, H / 3), (W / 3, -3), (2 * W / 3, H + 2), (W / 4, 3 * H / 4))
    rows = []
    for li, n in enumerate(LENGTHS):
        for ai, ang in enumerate(ANGLES):
            mx, my = centres[(li * len(ANGLES) + ai) % len(centres)]
            rows.append(S._around(mx + 0.25 * ai, my + 0.5 * li, ang, n) + (ang, n))
    return S.keylines(rows)


@functools.lru_cache(maxsize=None)
def _given(oracle, W, H, i):
    """(image, key lines, oracle descriptors) of image i of a batch, the same in every batch size"""
    img = np.roll(S.image(KINDS[i % len(KINDS)], W, H, 60 + i), i, axis=1)
    pool = _pool(W, H)
    kls = pool[(np.arange(_count(i)) * 7 + 11 * i) % len(pool)]      # (7 and 50 are coprime: distinct rows)
    return img, kls, oracle.lbd_compute(img, kls) if len(kls) else np.zeros((0, 32), np.uint8)


def test_given_lines_cover_the_cases():
    for W, H in SIZES:
        pool = _pool(W, H)
        used = np.concatenate([(np.arange(_count(i)) * 7 + 11 * i) % len(pool) for i in range(17)])
        k = pool[used]
        assert set(S.short_len(k).tolist()) == set(LENGTHS)
        flat = S.flat_side(k)
        assert flat.any() and (~flat).any()
        mx, my = (k["sPointInOctaveX"] + k["ePointInOctaveX"]) / 2, (k["sPointInOctaveY"] + k["ePointInOctaveY"]) / 2
        assert (mx < 0).any() and (mx > W - 1).any() and (my < 0).any() and (my > H - 1).any()
    assert {_count(i) for i in range(7)} == {0, 1, 3, 4, 5, CAP} and _count(1) == 0


@pytest.mark.parametrize("n", N_IMAGES)
@pytest.mark.parametrize("W,H", SIZES)
def test_given_key_lines(oracle, W, H, n):
    data = [_given(oracle, W, H, i) for i in range(n)]
    kl = np.stack([S.poison(CAP) for _ in range(n)])            # far key lines past every image's count: they must not be described
    counts = np.array([len(d[1]) for d in data], np.int32)
    for i, d in enumerate(data):
        kl[i, :counts[i]] = d[1]
    got = _extractor(n).compute_batch(np.stack([d[0] for d in data]), kl, counts)
    for i, d in enumerate(data):
        bad = np.flatnonzero((got[i, :counts[i]] != d[2]).any(1))
        assert len(bad) == 0, f"image {i} of {n}: rows {bad.tolist()} of {counts[i]} differ"


# ---- the detector's key lines -----------------------------------------------------------------------------------------------------------------------

def stairs(W, H, k, ang):
    """k parallel step edges across the image, normal direction ang"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = (x - W / 2) * np.cos(ang) + (y - H / 2) * np.sin(ang)
    span = 0.8 * min(W, H)
    img = np.full((H, W), 40.0)
    for i in range(k):
        img += (d > -span / 2 + span * (i + 0.5) / k) * (180.0 / k)
    return np.clip(img, 0, 255).astype(np.uint8)


STAIR_ANGLES = (0.77, 0.80, 0.3, 1.2, 2.0)                       # 0.77 and 0.80: either side of pi / 4


@functools.lru_cache(maxsize=None)
def _stairs_run(oracle, W, H, k, ai):
    img = stairs(W, H, k, STAIR_ANGLES[ai])
    return img, oracle.line_extract(img, oracle.full_params(2000, CAP).line)


@functools.lru_cache(maxsize=None)
def _detected(oracle, W, H, i):
    """(image, oracle run) of image i: the first staircase, angles taken in an order that depends on i, on which the oracle's detector keeps _count(i) lines"""
    want = _count(i)
    for da in range(len(STAIR_ANGLES)):
        for k in ((8, 7, 9) if want == CAP else (want, want + 1, want - 1) if want else (0,)):
            img, o = _stairs_run(oracle, W, H, k, (i + da) % len(STAIR_ANGLES))
            if len(o["kls"]) == want:
                return img, o
    raise AssertionError(f"no staircase with {want} detected lines at {W} x {H}")


def test_detected_lines_cover_the_cases(oracle):
    for W, H in SIZES:
        kls = np.concatenate([_detected(oracle, W, H, i)[1]["kls"] for i in range(17)])
        flat = S.flat_side(kls)
        assert flat.any() and (~flat).any()
        assert len({int(v) % 16 for v in kls["numOfPixels"]}) >= 4      # several tails of the 16-sample step


@pytest.mark.parametrize("n", N_IMAGES)
@pytest.mark.parametrize("W,H", SIZES)
def test_detected_key_lines(oracle, W, H, n):
    data = [_detected(oracle, W, H, i) for i in range(n)]
    kls, desc, counts = _extractor(n).extract_batch(np.stack([d[0] for d in data]))
    assert counts.tolist() == [_count(i) for i in range(n)]
    for i, (_, o) in enumerate(data):
        c = int(counts[i])
        for f in ("numOfPixels", "class_id"):
            assert np.array_equal(kls[i, :c][f], o["kls"][f]), (i, f)
        for f in ("angle", "sPointInOctaveX", "sPointInOctaveY", "ePointInOctaveX", "ePointInOctaveY"):
            assert np.array_equal(kls[i, :c][f].view(np.uint32), o["kls"][f].view(np.uint32)), (i, f)
        bad = np.flatnonzero((desc[i, :c] != o["desc"]).any(1))
        assert len(bad) == 0, f"image {i} of {n}: rows {bad.tolist()} of {c} differ"
