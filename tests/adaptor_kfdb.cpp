// KeyFrameDatabaseOf<KeyFrame, Frame> of include/orbline_reference_api.hpp on stand-in KeyFrame / Frame types that carry the members the template reads
// (mBowVec, mBowVec_l, mnId, N, N_l, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames), and ORBVocabulary::score.  Compiling it instantiates every
// member; running it needs a device (tests/test_kfdb_gpu.py): prints ADAPTOR_KFDB_OK.  Without one it prints ADAPTOR_KFDB_NEEDS_A_DEVICE and returns 77.
#include "../include/orbline_adaptor.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>

namespace standin {
typedef std::map<unsigned, double> BowVector;      // DBoW2::BowVector
struct KeyFrame {
    long unsigned int mnId = 0;
    int N = 0, N_l = 0;
    BowVector mBowVec, mBowVec_l;
    std::set<KeyFrame*> connected;
    std::vector<KeyFrame*> covisibles;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) { return std::vector<KeyFrame*>(covisibles.begin(), covisibles.begin() + std::min<size_t>(n, covisibles.size())); }
};
struct Frame {
    long unsigned int mnId = 0;
    int N = 0, N_l = 0;
    BowVector mBowVec, mBowVec_l;
};
}  // namespace standin
using namespace standin;
typedef ORB_SLAM2::KeyFrameDatabaseOf<KeyFrame, Frame> KeyFrameDatabase;

static BowVector uniform(unsigned first, unsigned last)
{
    BowVector v;
    for (unsigned w = first; w < last; ++w) v[w] = 1.0 / (last - first);
    return v;
}

// the database takes its sizes and scorings from vocabularies: the smallest real one, a root with `leaves` word children, as a DBoW2 text file
static bool write_voc(const char* path, int leaves)
{
    FILE* f = std::fopen(path, "w");
    if (!f) return false;
    std::fprintf(f, "%d 1 0 0\n", leaves);                      // k L scoring(L1_NORM) weighting(TF_IDF)
    for (int i = 0; i < leaves; ++i) {
        std::fprintf(f, "0 1");
        for (int b = 0; b < 32; ++b) std::fprintf(f, " %d", b == 0 ? i : 0);
        std::fprintf(f, " 1.0\n");
    }
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (olf_device_count() <= 0) { std::printf("ADAPTOR_KFDB_NEEDS_A_DEVICE\n"); return 77; }
    const std::string path = std::string(argc > 1 ? argv[1] : ".") + "/adaptor_kfdb_voc.txt";
    try {
        if (!write_voc(path.c_str(), 19)) return 2;
        ORB_SLAM2::ORBVocabulary voc, voc_l;
        // (the text loader reads one phantom node after the last newline, a childless child of the root that is not a word: 19 words)
        if (!voc.loadFromTextFile(path) || !voc_l.loadFromTextFile(path) || voc.size() != 19u) { std::printf("vocabulary: %u words\n", voc.size()); return 3; }
        KeyFrameDatabase db(voc, voc_l);
        KeyFrame A, B, C;
        A.mBowVec = uniform(0, 10); B.mBowVec = uniform(0, 9); B.mBowVec[12] = 0.0; C.mBowVec = uniform(10, 19);
        A.mBowVec_l = uniform(0, 4); B.mBowVec_l = uniform(0, 4); C.mBowVec_l = uniform(4, 8);
        db.add(&A); db.add(&B); db.add(&C);
        // relocalisation: the frame is A's copy.  A scores 1, B (9 common words of A's 10) about 0.9; both pass 0.75 of the best
        Frame F;
        F.mnId = 3; F.mBowVec = A.mBowVec; F.mBowVec_l = A.mBowVec_l; F.N = 100; F.N_l = 20;
        std::vector<KeyFrame*> r = db.DetectRelocalizationCandidates(&F);
        if (r.size() != 2 || r[0] != &A || r[1] != &B) { std::printf("reloc: %zu candidates\n", r.size()); return 4; }
        F.mnId = 4;
        r = db.DetectRelocalizationCandidatesWithLine(&F);
        if (r.size() != 2 || r[0] != &A || r[1] != &B) { std::printf("reloc with line: %zu candidates\n", r.size()); return 5; }
        // loop: the query key frame is connected to A, so B is what is left; with B's neighbour A ignored (connected), B stands alone
        KeyFrame Q;
        Q.mnId = 7; Q.mBowVec = A.mBowVec; Q.mBowVec_l = A.mBowVec_l; Q.N = 100; Q.N_l = 20; Q.connected.insert(&A);
        B.covisibles.push_back(&A);
        r = db.DetectLoopCandidates(&Q, 0.5f);
        if (r.size() != 1 || r[0] != &B) { std::printf("loop: %zu candidates\n", r.size()); return 6; }
        Q.mnId = 8;
        r = db.DetectLoopCandidatesWithLine(&Q, 0.5f);
        if (r.size() != 1 || r[0] != &B) { std::printf("loop with line: %zu candidates\n", r.size()); return 7; }
        // a repeated id is refused
        bool threw = false;
        try { db.DetectLoopCandidates(&Q, 0.5f); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) return 8;
        db.erase(&B);
        Q.mnId = 9;
        if (!db.DetectLoopCandidates(&Q, 0.5f).empty()) return 9;
        db.clear();
        F.mnId = 1;
        if (!db.DetectRelocalizationCandidates(&F).empty()) return 10;
        // TemplatedVocabulary::score: one common word of three, |0.25 - 0.5| - 0.25 - 0.5 = -0.5, score 0.25
        BowVector a, b;
        a[1] = 0.5; a[2] = 0.25; a[3] = 0.25; b[3] = 0.5; b[7] = 0.25; b[9] = 0.25;
        olf_ctx* ctx = nullptr;
        olf_params p;
        olf_default_params(&p);
        if (olf_ctx_create(&p, 640, 480, 1, &ctx) != OLF_OK) return 11;
        const double s = voc.score(ctx, a, b), s0 = voc.score(ctx, a, BowVector());
        olf_ctx_destroy(ctx);
        if (s != 0.25 || s0 != 0.0 || !std::signbit(s0)) { std::printf("score %.17g %.17g\n", s, s0); return 12; }
    } catch (const std::runtime_error& e) { std::printf("threw: %s\n", e.what()); return 20; }
    std::remove(path.c_str());
    std::printf("ADAPTOR_KFDB_OK\n");
    return 0;
}
