"""GPU parity: olf_search_by_bow_pairs_dev -- both ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cc:161-290, :524-657) for a list of key-frame pairs of
a device-resident batch, Frame::ComputeBoW included -- against the CPU oracle's two searches on the oracle's own feature vectors, pair by pair.  Equality
is exact.  The frames of all tests but the last two are fabricated (the entry takes arbitrary device arrays); the cases come from bow_pairs_scenes.py, whose
scenario_* functions assert that each case occurs (tests/test_bow_pairs_cpu.py runs those checks without a device)."""
import types
import numpy as np
import pytest
import bow_pairs_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_CAPACITY, lib
from bow_pairs_scenes import KF_FRAME, KF_KF
from status_text import describes

pytestmark = pytest.mark.gpu

W, H = 320, 240
FORMS = [KF_FRAME, KF_KF]


def test_form_constants():
    assert (matcher.BOW_KF_FRAME, matcher.BOW_KF_KF) == (KF_FRAME, KF_KF)


@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 400
    c = _lib.Context(p, W, H, 2)
    assert 400 <= c.orb_capacity <= 4096
    yield c
    c.close()


class DeviceFrames:
    """fabricated frames as device arrays in the extractor's layout; rows nothing may read hold random descriptors, a count of 17 and no map point"""

    def __init__(self, ctx, frames, img_stride=1):
        import torch
        cap, nf = ctx.orb_capacity, len(frames)
        self.ctx, self.n, self.st, self.cap = ctx, nf, img_stride, cap
        rng = np.random.default_rng(5)
        kps = np.zeros((nf * img_stride, cap), KEYPOINT_DTYPE)
        kps["angle"] = rng.uniform(0, 360, kps.shape)
        desc = rng.integers(0, 256, (nf * img_stride, cap, 32), dtype=np.uint8)
        cnt = np.full(nf * img_stride, 17, np.int32)
        valid, bad = np.zeros((nf, cap), np.uint8), np.ones((nf, cap), np.uint8)
        for j, fr in enumerate(frames):
            m = len(fr.keys)
            assert m <= cap
            kps[j * img_stride, :m], desc[j * img_stride, :m], cnt[j * img_stride] = fr.keys, fr.desc, m
            valid[j, :m], bad[j, :m] = fr.valid, fr.bad
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.desc, self.counts = up(kps.view(np.uint8).reshape(nf * img_stride, cap, 28)), up(desc), up(cnt)
        self.valid, self.bad = up(valid), up(bad)

    def search(self, G, pairs, form, levelsup, nnratio=0.7, check=True, masks=True, n_pairs=None):
        """(matches [len(pairs) + 1, cap], nmatches [len(pairs) + 1]) as numpy arrays: the outputs start as -7, the last row is a sentinel"""
        import torch
        P = len(pairs)
        d_pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(P, 2))).cuda()
        if n_pairs is not None:
            d_pairs = d_pairs[:n_pairs]
        out = (torch.full((P + 1, self.cap), -7, dtype=torch.int32, device="cuda"), torch.full((P + 1,), -7, dtype=torch.int32, device="cuda"))
        matcher.search_by_bow_pairs(G, self.n, self.kps, self.desc, self.counts, d_pairs, mp_valid=self.valid if masks else None,
                                    mp_bad=self.bad if masks else None, form=form, nnratio=nnratio, checkOri=check, levelsup=levelsup, img_stride=self.st,
                                    out=out, context=self.ctx)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()


def assert_rows(m, nm, exp, at=None):
    for p, (n_o, row_o) in enumerate(exp):
        q = p if at is None else at[p]
        assert nm[q] == n_o, (q, nm[q], n_o)
        assert np.array_equal(m[q, :len(row_o)], row_o), (q, int(np.argmax(m[q, :len(row_o)] != row_o)))
        assert (m[q, len(row_o):] == -1).all()


# 1 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [0, 1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,L,levelsup", S.TREES)
def test_all_ordered_pairs(ctx, k, L, levelsup, form, check):
    """every (i, j), i != j, of six frames with 0, 1, 63, 64, 65 and 300 features; the node level is the root, the leaves, and one between"""
    frames, voc, exp = S.scenario_all_pairs(k, L, levelsup, form, bool(check))
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, S.ALL_PAIRS, form, levelsup, check=bool(check))
    assert_rows(m, nm, exp)
    assert (m[-1] == -7).all() and nm[-1] == -7
    ctx.poll_status()
    G.clear()


@pytest.mark.parametrize("form", FORMS)
def test_null_masks(ctx, form):
    """mp_valid = NULL and d_mp_bad = NULL: every feature holds a good point"""
    frames, voc, exp = S.scenario_all_pairs(4, 3, 1, form, True, False)
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames, img_stride=2).search(G, S.ALL_PAIRS, form, 1, masks=False)
    assert_rows(m, nm, exp)
    G.clear()


# 2 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1.2, 0.9])
@pytest.mark.parametrize("form", FORMS)
def test_ties_and_chunks(ctx, form, ratio):
    """equal minima inside a chunk of 64 candidates and across chunks: the earlier candidate stays (ratio 1.2 shows the winner, 0.9 fails the test)"""
    frames, voc, pairs, exp = S.scenario_ties()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, pairs, form, 2, nnratio=ratio)
    assert_rows(m, nm, exp[form, ratio])
    G.clear()


# 3, 4 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_thresholds(ctx, form):
    """bestDist1 == TH_LOW is accepted by the frame form only; 30 against 0.75 * 40 fails the ratio test"""
    frames, voc, pairs, exp = S.scenario_thresholds()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, pairs, form, 2, nnratio=0.75)
    assert_rows(m, nm, exp[form])
    G.clear()


@pytest.mark.parametrize("form", FORMS)
def test_greedy_state(ctx, form):
    """a feature of the second frame that is taken is passed over by the next feature of the first frame in the node"""
    frames, voc, pairs, exp = S.scenario_greedy()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, pairs, form, 2, nnratio=0.75, check=False)
    assert_rows(m, nm, exp[form])
    G.clear()


# 5 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_rotation_drops(ctx, form):
    frames, voc, pairs, exp = S.scenario_rotation()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, pairs, form, 1)
    assert_rows(m, nm, exp[form])
    G.clear()


# 6 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_pair_list_edges_in_one_call(ctx, form):
    """a duplicate pair, a pair in both orders, one frame in eight pairs; indices -1 and n_frames and equal indices between them"""
    frames, voc, pairs, good_at, bad_at, exp = S.scenario_edges(form)
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    dev = DeviceFrames(ctx, frames)
    ctx.poll_status()
    m, nm = dev.search(G, pairs, form, 1)
    for q in bad_at:
        assert nm[q] == -1 and (m[q] == -7).all()
    assert_rows(m, nm, exp, good_at)
    assert (m[-1] == -7).all() and nm[-1] == -7              # nothing past either output array
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=2048" in str(e.value) and describes(e.value, 2048)
    ctx.poll_status()                                       # reported once, then clear
    for bad in S.EDGE_BAD[:3]:                              # each kind alone: -1, n_frames, equal
        m, nm = dev.search(G, [bad], form, 1)
        assert nm[0] == -1 and (m == -7).all()
        with pytest.raises(ola.OlfError) as e:
            ctx.poll_status()
        assert "flags=2048" in str(e.value) and describes(e.value, 2048)
    m, nm = dev.search(G, [(5, 4)], form, 1, n_pairs=0)      # n_pairs = 0 writes nothing
    assert (m == -7).all() and (nm == -7).all()
    ctx.poll_status()
    G.clear()


# 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_consecutive_pairs_equal_the_batch_entry(ctx, stride):
    """OLF_BOW_KF_FRAME over (j, j + 1) equals olf_search_by_bow_batch_dev on the same arrays, rows and counts"""
    import torch
    frames, voc, pairs, exp = S.scenario_consecutive()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    dev = DeviceFrames(ctx, frames, img_stride=stride)
    m, nm = dev.search(G, pairs, KF_FRAME, 1)
    assert_rows(m, nm, exp)
    P = len(pairs)
    om, on = torch.full((P, dev.cap), -7, dtype=torch.int32, device="cuda"), torch.full((P,), -7, dtype=torch.int32, device="cuda")
    with matcher._torch_stream() as s:
        _lib.check(lib().olf_search_by_bow_batch_dev(ctx.handle, G._h, dev.n, stride, dev.kps.data_ptr(), dev.desc.data_ptr(), dev.counts.data_ptr(),
                                                     dev.valid.data_ptr(), dev.bad.data_ptr(), 0.7, 1, 1, om.data_ptr(), on.data_ptr(), s),
                   "olf_search_by_bow_batch_dev")
    torch.cuda.synchronize()
    assert np.array_equal(om.cpu().numpy(), m[:P]) and np.array_equal(on.cpu().numpy(), nm[:P])
    G.clear()


# 8 -----------------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    """a context above 4096 features per frame is refused before any launch"""
    import ctypes as C
    import torch
    p = _lib.default_params()
    p.orb.nfeatures = 4097
    big = _lib.Context(p, W, H, 1)
    try:
        assert big.orb_capacity > 4096
        voc, _, _ = S.make_voc(4, 2, S.frames6()[1])
        G = ola.ORBVocabulary.from_arrays(*voc, context=big)
        buf = torch.full((64,), -7, dtype=torch.int32, device="cuda")
        tb = _lib.TrackBatchC()
        tb.kps, tb.desc, tb.counts, tb.img_stride = buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1
        rc = lib().olf_search_by_bow_pairs_dev(big.handle, G._h, C.byref(tb), 2, 1, buf.data_ptr(), None, KF_FRAME, 0.7, 1, 4, buf.data_ptr(), buf.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == OLF_ERR_CAPACITY and "olf_search_by_bow_pairs_dev" in _lib.last_error()
        assert (buf == -7).all()                            # (refused before anything is read or written)
        G.clear()
    finally:
        big.close()


# 9, 10: extracted frames ---------------------------------------------------------------------------------------------------------------------
PAIRS3 = [(i, j) for i in range(3) for j in range(3) if i != j]


@pytest.fixture(scope="module")
def extracted(oracle):
    """3 synthetic stereo pairs, shifted copies of one scene, through the extractor (img_stride 2); masks from olf_stereo_points_mask_dev; the oracle's
    results for the 6 ordered pairs in both forms"""
    import torch
    from orb_line_slam_amd import synth
    w, h, B = 640, 480, 3
    fe = ola.StereoFrontEnd(oracle.full_params(1000, 100), w, h, max_pairs=B)
    imgs = synth.stereo_batch(67, B, w, h)
    for i in range(1, B):
        imgs[2 * i:2 * i + 2] = np.roll(imgs[:2], 3 * i, axis=2)
    f = fe.frames(imgs)
    src = np.concatenate([f.pair(i)["mDescriptors"] for i in range(B)])
    parent, leaf, vdesc, weight = oracle.random_vocabulary(10, 3, 8)
    vdesc[1:] = src[np.random.default_rng(1).integers(0, len(src), len(parent) - 1)]
    G = ola.ORBVocabulary.from_arrays(10, 3, parent, leaf, vdesc, weight)
    V = oracle.OracleVoc.create(10, 3, parent, leaf, vdesc, weight)
    mask = fe.stereo_points_mask()
    views = []
    for i in range(B):
        g = f.pair(i)
        fr = S.frame(g["mDescriptors"], valid=g["mvDepth"] > 0)
        fr.keys = g["mvKeys"]
        views.append(S.view(fr, V, 2))
    run = lambda form: fe.search_by_bow_pairs(G, np.asarray(PAIRS3, np.int32), mp_valid=mask, form=form, nnratio=0.7, levelsup=2)
    got, exp = {}, {}
    for form in FORMS:
        m, nm = run(form)
        torch.cuda.synchronize()
        got[form] = (m.cpu().numpy(), nm.cpu().numpy())
        exp[form] = S.oracle_pairs(views, PAIRS3, form, 0.7, True)
    yield types.SimpleNamespace(fe=fe, G=G, mask=mask, run=run, got=got, exp=exp, B=B)
    G.clear()
    fe.ctx.close()


@pytest.mark.parametrize("form", FORMS)
def test_extracted_frames_stride_2(extracted, form):
    e = extracted
    assert sum(n for n, _ in e.exp[form]) > 30 * len(PAIRS3)
    assert_rows(*e.got[form], e.exp[form])


def test_shared_scratch_and_stage(extracted):
    """SearchByBoW over consecutive frames, the pair list in both forms, SearchByBoW again, on one stream: all share the FeatureVector stage and the
    context's batch scratch"""
    import torch
    e = extracted
    fb, B = e.fe._last_frames("test")
    cap, h = e.fe.ctx.orb_capacity, e.fe.ctx.handle
    bow = [(torch.full((B - 1, cap), -7, dtype=torch.int32, device="cuda"), torch.full((B - 1,), -7, dtype=torch.int32, device="cuda")) for _ in range(2)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        call = lambda o: _lib.check(lib().olf_search_by_bow_batch_dev(h, e.G._h, B, 2, fb.kps, fb.desc, fb.counts, e.mask.data_ptr(), None, 0.7, 1, 2,
                                                                      o[0].data_ptr(), o[1].data_ptr(), s), "olf_search_by_bow_batch_dev")
        call(bow[0])
        mid = {form: e.run(form) for form in FORMS}
        call(bow[1])
    torch.cuda.synchronize()
    assert torch.equal(bow[0][0], bow[1][0]) and torch.equal(bow[0][1], bow[1][1]) and int(bow[0][1].sum()) > 0
    for form in FORMS:
        assert np.array_equal(mid[form][0].cpu().numpy(), e.got[form][0]) and np.array_equal(mid[form][1].cpu().numpy(), e.got[form][1])
    # the consecutive pairs of the batch entry are pairs 0 -> 1 and 1 -> 2 of the list
    m, nm = e.got[KF_FRAME]
    for j in range(B - 1):
        q = PAIRS3.index((j, j + 1))
        assert np.array_equal(bow[0][0][j].cpu().numpy(), m[q]) and int(bow[0][1][j]) == nm[q]
