// FrameGrid(F) of include/orbline_reference_api.hpp on a stand-in Frame that carries the members the template reads (mvKeysUn, mnMinX .. mnMaxY) and
// the one it fills (mGrid, include/Frame.h:228): the cells must equal a host loop of Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:334-349,
// :572-582) written here, and flatten into a grid a C-ABI search accepts.  Needs a device (run by tests/test_grid_gpu.py): prints FRAME_GRID_OK.
#include "../include/orbline_adaptor.hpp"
#include <cmath>
#include <cstdio>

namespace standin {
typedef olf_keypoint KeyPoint;          // layout of cv::KeyPoint
struct Frame {
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<std::size_t> mGrid[OLF_GRID_COLS][OLF_GRID_ROWS];
};
float Frame::mnMinX = -11.5f, Frame::mnMaxX = 1250.25f, Frame::mnMinY = -7.f, Frame::mnMaxY = 380.5f;      // undistorted bounds: not the image's
}  // namespace standin
using standin::Frame;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

static void fill(Frame& F, int n)
{
    F.N = n;
    F.mvKeysUn.resize(n);
    for (int i = 0; i < n; ++i) {
        olf_keypoint k = {};
        // quarter-pixel positions from 8 px outside the bounds on every side: some keys fall out of the grid, many products are exact ties
        k.x = Frame::mnMinX - 8.f + 0.25f * (float)(rnd() % (4 * 1280)); k.y = Frame::mnMinY - 8.f + 0.25f * (float)(rnd() % (4 * 404));
        k.octave = (int)(rnd() % 8); k.size = 31.f; k.class_id = -1;
        F.mvKeysUn[i] = k;
    }
}

// Frame::AssignFeaturesToGrid as the reference writes it
static void host_grid(const Frame& F, std::vector<std::size_t> (*grid)[OLF_GRID_ROWS])
{
    const float wInv = static_cast<float>(OLF_GRID_COLS) / (Frame::mnMaxX - Frame::mnMinX), hInv = static_cast<float>(OLF_GRID_ROWS) / (Frame::mnMaxY - Frame::mnMinY);
    for (int i = 0; i < F.N; i++) {
        const olf_keypoint& kp = F.mvKeysUn[i];
        const int posX = (int)std::round((kp.x - Frame::mnMinX) * wInv), posY = (int)std::round((kp.y - Frame::mnMinY) * hInv);
        if (posX < 0 || posX >= OLF_GRID_COLS || posY < 0 || posY >= OLF_GRID_ROWS) continue;
        grid[posX][posY].push_back(i);
    }
}

static int check_frame(int n)
{
    Frame F;
    fill(F, n);
    static std::vector<std::size_t> want[OLF_GRID_COLS][OLF_GRID_ROWS];
    for (auto& col : want) for (auto& cell : col) cell.clear();
    host_grid(F, want);
    F.mGrid[3][5].assign(7, 99);                                   // stale content must not survive
    ORB_SLAM2::FrameGrid(F);
    std::size_t kept = 0;
    for (int i = 0; i < OLF_GRID_COLS; ++i)
        for (int j = 0; j < OLF_GRID_ROWS; ++j) {
            if (F.mGrid[i][j] != want[i][j]) { std::printf("n = %d: cell (%d, %d) differs (%zu vs %zu entries)\n", n, i, j, F.mGrid[i][j].size(), want[i][j].size()); return 1; }
            kept += want[i][j].size();
        }
    if (n >= 100 && (kept == 0 || kept == (std::size_t)n)) { std::printf("n = %d: %zu keys kept -- the case is meant to drop some\n", n, kept); return 2; }
    // flattened, the member is the grid of orbline_types.h
    const ORB_SLAM2::olf_detail::GridCSR csr(F);
    if ((int)csr.offs.size() != OLF_GRID_CELLS + 1 || csr.offs.back() != (int32_t)kept || csr.idx.size() != kept) return 3;
    for (int e = 0; e < OLF_GRID_CELLS; ++e)
        for (int k = csr.offs[e]; k < csr.offs[e + 1]; ++k) if ((std::size_t)csr.idx[k] != want[e / OLF_GRID_ROWS][e % OLF_GRID_ROWS][k - csr.offs[e]]) return 4;
    olf_frame_view v = olf_frame_view();
    csr.attach(v);
    if (v.grid_offsets != csr.offs.data() || v.grid_index != csr.idx.data()) return 5;
    return 0;
}

int main()
{
    if (olf_device_count() <= 0) { std::printf("FRAME_GRID_NEEDS_A_DEVICE\n"); return 77; }
    try {
        const int sizes[] = {0, 1, 64, 777, 2000};
        for (int n : sizes) { const int rc = check_frame(n); if (rc) return rc; }
        // beyond the documented limit the call is refused, not truncated
        Frame big; fill(big, OLF_GRID_MAX_KEYS + 1);
        bool threw = false;
        try { ORB_SLAM2::FrameGrid(big); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("FrameGrid accepted OLF_GRID_MAX_KEYS + 1 key points\n"); return 6; }
    } catch (const std::runtime_error& e) { std::printf("threw: %s\n", e.what()); return 20; }
    std::printf("FRAME_GRID_OK\n");
    return 0;
}
