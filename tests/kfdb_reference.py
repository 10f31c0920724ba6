"""A pure-Python restatement of the reference's place recognition, written from the reference's source and used as the oracle of the key-frame database
tests (the reference's DBoW2 scoring cannot be compiled without OpenCV: ScoringObject.cpp pulls it in through TemplatedVocabulary.h):

    L1Scoring::score                                         Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
    KeyFrameDatabase::add / erase / clear                    src/KeyFrameDatabase.cc:46-98
    KeyFrameDatabase::DetectLoopCandidates                   :107-228
    KeyFrameDatabase::DetectLoopCandidatesWithLine           :230-400
    KeyFrameDatabase::DetectRelocalizationCandidates         :402-512
    KeyFrameDatabase::DetectRelocalizationCandidatesWithLine :514-667

The inverted file is a real list per word, the per-key-frame members are attributes initialised as src/KeyFrame.cc:35-37, the double chain of the score
is Python floats and every `float` of the reference is a numpy.float32.  Where the reference iterates a std::set<KeyFrame*> (address order) the key
frames' `addr` stands for the address: the order of construction.
"""
import bisect
import itertools
import numpy as np

f32 = np.float32


def l1_score(v1, v2):
    """ScoringObject.cpp:23-68.  v1, v2: BowVectors as lists of (word id, value) in ascending id (a std::map)"""
    k1, k2 = [w for w, _ in v1], [w for w, _ in v2]
    i1, i2 = 0, 0                                                    # :29-30
    score = 0.0                                                      # :32
    while i1 != len(v1) and i2 != len(v2):                           # :34
        vi, wi = v1[i1][1], v2[i2][1]                                # :36-37
        if k1[i1] == k2[i2]:                                         # :39
            score += abs(vi - wi) - abs(vi) - abs(wi)                # :41
            i1 += 1                                                  # :44-45
            i2 += 1
        elif k1[i1] < k2[i2]:                                        # :47
            i1 = bisect.bisect_left(k1, k2[i2])                      # :50 lower_bound
        else:
            i2 = bisect.bisect_left(k2, k1[i1])                      # :56
    score = -score / 2.0                                             # :65
    return score


_addr = itertools.count(1)


class KeyFrame:
    """the members of KeyFrame (and of Frame, for a query) that KeyFrameDatabase.cc reads and writes"""

    def __init__(self, mnId, bow, bow_l=(), N=0, N_l=0, name=None):
        self.name, self.addr = name, next(_addr)
        self.mnId, self.N, self.N_l = mnId, N, N_l
        self.mBowVec = sorted(dict(bow).items())
        self.mBowVec_l = sorted(dict(bow_l).items())
        # src/KeyFrame.cc:35-37
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore, self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, f32(0), 0, 0, f32(0)
        self.mnLoopQuery_l, self.mnLoopWords_l, self.mLoopScore_l, self.mnRelocQuery_l, self.mnRelocWords_l, self.mRelocScore_l = 0, 0, f32(0), 0, 0, f32(0)
        self.mLoopScore_pl, self.mRelocScore_pl = f32(0), f32(0)
        self.connected = set()          # GetConnectedKeyFrames()
        self.best_covisibles = []       # GetBestCovisibilityKeyFrames(10), in order

    def GetConnectedKeyFrames(self):
        return set(self.connected)

    def GetBestCovisibilityKeyFrames(self, n):
        return list(self.best_covisibles[:n])


class Vocabulary:
    def __init__(self, n_words):
        self.n_words = n_words

    def size(self):
        return self.n_words

    def empty(self):
        return self.n_words == 0

    def score(self, a, b):
        return l1_score(a, b)


class KeyFrameDatabase:
    def __init__(self, voc, voc_l):                                  # :39-44
        self.mpVoc, self.mpVoc_l = voc, voc_l
        self.mvInvertedFile = [[] for _ in range(voc.size())]
        self.mvInvertedFile_l = [[] for _ in range(voc_l.size())]

    def add(self, pKF):                                              # :46-55
        for w, _ in pKF.mBowVec:
            self.mvInvertedFile[w].append(pKF)
        for w, _ in pKF.mBowVec_l:
            self.mvInvertedFile_l[w].append(pKF)

    def erase(self, pKF):                                            # :57-90
        for w, _ in pKF.mBowVec:
            lKFs = self.mvInvertedFile[w]
            for i, kf in enumerate(lKFs):
                if kf is pKF:
                    del lKFs[i]
                    break
        for w, _ in pKF.mBowVec_l:
            lKFs = self.mvInvertedFile_l[w]
            for i, kf in enumerate(lKFs):
                if kf is pKF:
                    del lKFs[i]
                    break

    def clear(self):                                                 # :92-98
        self.mvInvertedFile = [[] for _ in range(self.mpVoc.size())]
        self.mvInvertedFile_l = [[] for _ in range(self.mpVoc_l.size())]

    # ------------------------------------------------------------------------------------------------------------------
    def DetectLoopCandidates(self, pKF, minScore):                   # :107-228
        minScore = f32(minScore)
        spConnectedKeyFrames = pKF.GetConnectedKeyFrames()           # :109
        lKFsSharingWords = []
        for w, _ in pKF.mBowVec:                                     # :117-135
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:                                     # :138
            return []
        lScoreAndMatch = []
        maxCommonWords = 0                                           # :144-149
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))         # :151
        for pKFi in lKFsSharingWords:                                # :156-170
            if pKFi.mnLoopWords > minCommonWords:
                si = f32(self.mpVoc.score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:                                       # :172
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore                                      # :176
        for s, pKFi in lScoreAndMatch:                               # :179-204
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = f32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)         # :206-227

    @staticmethod
    def _retain(lAccScoreAndMatch, bestAccScore):                    # :206-227, :378-399, :492-511, :647-666
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF, out = set(), []
        for s, pKFi in lAccScoreAndMatch:
            if s > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    out.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        return out

    def DetectLoopCandidatesWithLine(self, pKF, minScore):           # :230-400
        minScore = f32(minScore)
        if self.mpVoc_l.empty():                                     # :232-235
            return []
        spConnectedKeyFrames = pKF.GetConnectedKeyFrames()
        lKFsSharingWords, lKFsSharingWords_l = [], []
        for w, _ in pKF.mBowVec:                                     # :246-264
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        for w, _ in pKF.mBowVec_l:                                   # :266-284
            for pKFi in self.mvInvertedFile_l[w]:
                if pKFi.mnLoopQuery_l != pKF.mnId:
                    pKFi.mnLoopWords_l = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery_l = pKF.mnId
                        lKFsSharingWords_l.append(pKFi)
                pKFi.mnLoopWords_l += 1
        if not lKFsSharingWords and not lKFsSharingWords_l:          # :287
            return []
        maxCommonWords = 0                                           # :291-297
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        maxCommonWords_l = 0                                         # :299-305
        for kf in lKFsSharingWords_l:
            if kf.mnLoopWords_l > maxCommonWords_l:
                maxCommonWords_l = kf.mnLoopWords_l
        minCommonWords_l = int(f32(maxCommonWords_l) * f32(0.8))
        sKFsSharingWords_pl = set()                                  # :307-323
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                sKFsSharingWords_pl.add(pKFi)
        for pKFi in lKFsSharingWords_l:
            if pKFi.mnLoopWords_l > minCommonWords_l:
                sKFsSharingWords_pl.add(pKFi)
        lScoreAndMatch = []
        np_, nl = pKF.N, pKF.N_l                                     # :327-328
        for pKFi in sorted(sKFsSharingWords_pl, key=lambda k: k.addr):   # :331-341, set order
            spi = f32(self.mpVoc.score(pKF.mBowVec, pKFi.mBowVec))
            sli = f32(self.mpVoc_l.score(pKF.mBowVec_l, pKFi.mBowVec_l))
            pKFi.mLoopScore, pKFi.mLoopScore_l = spi, sli
            pKFi.mLoopScore_pl = _combined(spi, sli, np_, nl)
            if pKFi.mLoopScore_pl > minScore:
                lScoreAndMatch.append((pKFi.mLoopScore_pl, pKFi))
        if not lScoreAndMatch:                                       # :343
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore                                      # :347
        for s, pKFi in lScoreAndMatch:                               # :350-376
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if (pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords
                        and pKF2.mnLoopQuery_l == pKF.mnId and pKF2.mnLoopWords_l > minCommonWords_l):
                    accScore = f32(accScore + pKF2.mLoopScore_pl)
                    if pKF2.mLoopScore_pl > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore_pl
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def DetectRelocalizationCandidates(self, F):                     # :402-512
        lKFsSharingWords = []
        for w, _ in F.mBowVec:                                       # :410-425
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:                                     # :427
            return []
        maxCommonWords = 0                                           # :431-438
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:                                # :445-456
            if pKFi.mnRelocWords > minCommonWords:
                si = f32(self.mpVoc.score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:                                       # :458
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)                                        # :462
        for s, pKFi in lScoreAndMatch:                               # :465-490
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnRelocQuery != F.mnId:                      # :476
                    continue
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def DetectRelocalizationCandidatesWithLine(self, F):             # :514-667
        if self.mpVoc_l.empty():                                     # :516-519
            return []
        lKFsSharingWords, lKFsSharingWords_l = [], []
        for w, _ in F.mBowVec:                                       # :528-543
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        for w, _ in F.mBowVec_l:                                     # :545-560
            for pKFi in self.mvInvertedFile_l[w]:
                if pKFi.mnRelocQuery_l != F.mnId:
                    pKFi.mnRelocWords_l = 0
                    pKFi.mnRelocQuery_l = F.mnId
                    lKFsSharingWords_l.append(pKFi)
                pKFi.mnRelocWords_l += 1
        if not lKFsSharingWords and not lKFsSharingWords_l:          # :562
            return []
        maxCommonWords = 0                                           # :566-572
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        maxCommonWords_l = 0                                         # :574-580
        for kf in lKFsSharingWords_l:
            if kf.mnRelocWords_l > maxCommonWords_l:
                maxCommonWords_l = kf.mnRelocWords_l
        minCommonWords_l = int(f32(maxCommonWords_l) * f32(0.8))
        sKFsSharingWords_pl = set()                                  # :582-596
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                sKFsSharingWords_pl.add(pKFi)
        for pKFi in lKFsSharingWords_l:
            if pKFi.mnRelocWords_l > minCommonWords_l:
                sKFsSharingWords_pl.add(pKFi)
        lScoreAndMatch = []
        np_, nl = F.N, F.N_l                                         # :600-601
        for pKFi in sorted(sKFsSharingWords_pl, key=lambda k: k.addr):   # :602-611, set order
            spi = f32(self.mpVoc.score(F.mBowVec, pKFi.mBowVec))
            sli = f32(self.mpVoc_l.score(F.mBowVec_l, pKFi.mBowVec_l))
            pKFi.mRelocScore, pKFi.mRelocScore_l = spi, sli
            pKFi.mRelocScore_pl = _combined(spi, sli, np_, nl)
            lScoreAndMatch.append((pKFi.mRelocScore_pl, pKFi))
        if not lScoreAndMatch:                                       # :613
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)                                        # :617
        for s, pKFi in lScoreAndMatch:                               # :620-645
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if not (pKF2.mnRelocQuery == F.mnId and pKF2.mnRelocQuery_l == F.mnId):     # :631
                    continue
                accScore = f32(accScore + pKF2.mRelocScore_pl)
                if pKF2.mRelocScore_pl > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore_pl
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)


def _combined(spi, sli, np_, nl):
    """(spi*np+sli*nl)/(np+nl), :338, :609: float * int is a float product, the int sum is converted to float for the division"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(f32(f32(spi * f32(np_)) + f32(sli * f32(nl))) / f32(np_ + nl))


def tables(queries, slots):
    """What olf_kfdb_tables_dev computes, from the definitions: for every (query vector, slot) the number of common words, the smallest common word (-1:
    none) and the L1 score (-0.0 where nothing is common).  queries, slots: BowVectors as sorted (id, value) lists; an erased slot is an empty list."""
    Q, n = len(queries), len(slots)
    common, first, score = np.zeros((Q, n), np.int32), np.full((Q, n), -1, np.int32), np.full((Q, n), -0.0, np.float64)
    for q, v in enumerate(queries):
        ids = {w for w, _ in v}
        for k, s in enumerate(slots):
            both = sorted(ids.intersection(w for w, _ in s))
            if both:
                common[q, k], first[q, k], score[q, k] = len(both), both[0], l1_score(v, s)
    return {"common": common, "first": first, "score": score}
