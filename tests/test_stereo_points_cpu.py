"""The constructed scenes of Frame::ComputeStereoMatches (tests/stereo_point_scenes.py) checked without a GPU: they are deterministic and in bounds, every
kind takes the branch it names (counted on the restatement's own outputs), the line-by-line restatement (tests/stereo_points_reference.py) and the CPU
oracle agree bit for bit, the hand-derived answers come out of both, and every named mutation of the restatement changes the answer on some scene --
i.e. the scenes would notice that mistake in a kernel."""
import collections
import numpy as np
import pytest
import stereo_point_scenes as S
import stereo_points_reference as ref

OUT = ("uRight", "depth")


def _mutated(s, mutation):
    try:
        return S.reference(s, mutate=mutation)
    except ref.SceneError:       # the mistake would read outside a level: as different as an answer can be
        return None


def _same(a, b):
    if a is None or b is None:
        return False
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in OUT) and np.array_equal(a["sad"], b["sad"])


def _all_scenes():
    return S.all_scenes() + [h[0] for h in S.hand_scenes()]


def test_scenes_are_deterministic_and_in_bounds(oracle):
    a, b = S._main(11, S.W, S.H, "again"), S.main_scene()
    for k in ("imgL", "imgR", "kpsL", "descL", "kpsR", "descR"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert S.max_disparity() == np.float32(S.BF) / (np.float32(S.BF) / np.float32(S.FX))
    sf, inv = S.tables()
    drawn = set()
    for s in _all_scenes():
        assert s["imgL"].shape == s["imgR"].shape == (s["h"], s["w"]) and s["imgL"].dtype == np.uint8
        lw, lh = oracle.orb_level_sizes(S.params().orb, s["w"], s["h"])
        assert len(s["kinds"]) == len(s["kpsL"]) == len(s["descL"]) and len(s["kpsR"]) == len(s["descR"])
        drawn |= set(s["kinds"])
        for side, k in (("L", s["kpsL"]), ("R", s["kpsR"])):
            for i in range(len(k)):
                o = int(k["octave"][i])
                assert 0 <= o < len(sf)
                xi, yi = ref.c_round(k["x"][i] * inv[o]), ref.c_round(k["y"][i] * inv[o])
                assert 16 <= yi <= lh[o] - 17, (s["name"], side, i)
                border = i in s["border_pts"][side]                        # (the border kind alone may stand nearer to the right edge)
                assert 16 <= xi <= lw[o] - (6 if border else 17), (s["name"], side, i)
    assert drawn == set(S.KINDS)
    assert [(len(s["kpsL"]), len(s["kpsR"])) for s in S.shape_scenes()] == S.SHAPES + [(S.capacity(), S.capacity())]
    assert S.scene_kinds(S.main_scene()) == S.main_scene()["kinds"]


def test_every_kind_takes_its_branch():
    met = collections.Counter()
    big = dropped = kept_near = 0
    for s in S.kind_scenes():
        r = s["ref"]
        assert s["whole"]
        for i, kind in enumerate(s["kinds"]):
            m = S.expectation_met(s, r, i)
            assert m is not False, (s["name"], i, kind, s["expect"][i], str(r["tag"][i]))
            met[kind] += bool(m)
        acc = np.flatnonzero(r["uRight"] >= 0)
        for i in acc:
            b = int(r["bestinc"][i]) + 5
            big += int(r["sads"][i, b - 1:b + 2].max()) >= 32768
        m = np.sort(r["sad"][r["sad"] >= 0])
        if len(m):
            th = np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(m[len(m) // 2])
            dropped += int((r["tag"] == "median").sum())
            kept_near += int(((r["tag"] == "ok") & (r["sad"] >= 0) & (np.abs(r["sad"].astype(np.float64) - float(th)) <= 1)).sum())
    for kind in S.KINDS:
        assert met[kind] >= 4, (kind, met[kind])
    assert big >= 8 and dropped >= 1 and kept_near >= 1, (big, dropped, kept_near)
    # a full scene (capacity x capacity): at most 10 % of the left points end without any candidate
    s = S.full_scene()
    r = s["ref"]
    none = (r["tag"] == "no_row_cand") | (r["tag"] == "maxU") | ((r["tag"] == "no_match") & (r["bestDist"] == ref.TH_HIGH))
    assert len(r["tag"]) == S.capacity() and none.sum() <= 0.1 * len(r["tag"]), none.sum()
    assert (r["uRight"] >= 0).sum() >= 0.5 * len(r["tag"])
    print("floors:", dict(met), "big", big, "dropped", dropped, "kept within 1", kept_near, "no candidate", int(none.sum()))


def test_restatement_equals_oracle():
    for s in _all_scenes():
        assert _same(s["ref"], S.oracle_answer(s)), s["name"]


def test_hand_scenes():
    hs = S.hand_scenes()
    assert len(hs) >= 6
    for s, ur, dp in hs:
        for got in (s["ref"], S.oracle_answer(s)):
            assert np.array_equal(got["uRight"].view(np.uint32), ur.view(np.uint32)), (s["name"], got["uRight"], ur)
            assert np.array_equal(got["depth"].view(np.uint32), dp.view(np.uint32)), (s["name"], got["depth"], dp)


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_mutation_is_caught(mutation):
    caught = [s["name"] for s in S.kind_scenes() + [h[0] for h in S.hand_scenes()] if not _same(_mutated(s, mutation), s["ref"])]
    print(mutation, "caught by", caught)
    assert caught, mutation
