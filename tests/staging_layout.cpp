// The offset arithmetic of the scratch carve (orb_line_slam_amd/csrc/carve.hpp), compiled alone with g++ -fsanitize=address,undefined and run as its own
// process by test_host_cpu.py.  For every request list: each region starts at a multiple of the alignment; regions lie in request order and do not
// overlap; a region of no elements has an address of its own; the total covers the last region.  Lists that fit are filled into a heap block of exactly
// total() bytes and the first and last byte of every region is written, so a region outside the block is the sanitizer's finding too.
#include "../orb_line_slam_amd/csrc/carve.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <size_t N> struct Blob { unsigned char b[N]; };
struct Req { size_t elem, count; };

static void add(olf::CarveLayout& k, size_t elem, void** slot, size_t count)
{
    switch (elem) {
    case 1: k.add(reinterpret_cast<Blob<1>**>(slot), count); break;
    case 2: k.add(reinterpret_cast<Blob<2>**>(slot), count); break;
    case 4: k.add(reinterpret_cast<Blob<4>**>(slot), count); break;
    case 8: k.add(reinterpret_cast<Blob<8>**>(slot), count); break;
    case 12: k.add(reinterpret_cast<Blob<12>**>(slot), count); break;
    case 16: k.add(reinterpret_cast<Blob<16>**>(slot), count); break;
    case 28: k.add(reinterpret_cast<Blob<28>**>(slot), count); break;
    default: std::abort();
    }
}

static int g_lists = 0;

static bool check(const std::vector<Req>& list, const char* what)
{
    ++g_lists;
    olf::CarveLayout k;
    void* ptr[olf::kCarveMaxRegions] = {};
    for (size_t i = 0; i < list.size(); ++i) add(k, list[i].elem, &ptr[i], list[i].count);
    const size_t total = k.total();
    const bool real = total <= ((size_t)64 << 20);
    // (a list too large to allocate is laid out from a made-up base: the pointers are compared, never followed)
    char* base = real ? static_cast<char*>(std::malloc(total)) : reinterpret_cast<char*>((uintptr_t)1 << 40);
    k.fill(base);
    bool ok = true;
    auto fail = [&](const char* why, size_t i) { std::printf("FAIL %s: region %zu %s\n", what, i, why); ok = false; };
    size_t end_prev = 0;
    for (size_t i = 0; i < list.size(); ++i) {
        if (!ptr[i]) { fail("was not filled", i); continue; }
        const size_t off = (size_t)(static_cast<char*>(ptr[i]) - base), bytes = list[i].elem * list[i].count;
        if (off % olf::kCarveAlign) fail("is not aligned", i);
        if (i == 0 && off != 0) fail("does not start the slab", i);
        if (off < end_prev) fail("overlaps the one before it or lies in front of it", i);
        for (size_t j = 0; j < i; ++j) if (ptr[j] == ptr[i]) fail("shares its address with another", i);
        if (off + bytes > total || off >= total) fail("is not covered by the total", i);
        else if (real && bytes) { static_cast<char*>(ptr[i])[0] = 1; static_cast<char*>(ptr[i])[bytes - 1] = 1; }
        end_prev = off + bytes;
    }
    if (total % olf::kCarveAlign) fail("total is not a multiple of the alignment", list.size());
    if (real) std::free(base);
    return ok;
}

int main()
{
    bool ok = true;
    const size_t elems[] = {1, 2, 4, 8, 12, 16, 28};
    const size_t counts[] = {0, 1, 3, 5, 7, 33, 1001};
    // one region of every element size and count, alone and in front of a second one
    for (size_t e : elems)
        for (size_t n : counts) { ok &= check({{e, n}}, "single"); ok &= check({{e, n}, {4, 1}}, "pair"); }
    // the shapes the entry points cut
    ok &= check({{1, 32}, {1, 32}, {4, 2}, {4, 3}}, "knn2 (1, 1)");
    ok &= check({{1, 5 * 32}, {1, 0}, {4, 2}, {4, 15}}, "knn2 (5, 0)");
    ok &= check({{1, 300 * 32}, {1, 4096 * 32}, {4, 2}, {4, 900}}, "knn2 (300, 4096)");
    ok &= check({{1, 96}, {1, 224}, {4, 4}, {4, 3}, {2, 3}}, "match_candidates, 3 candidates");
    ok &= check({{28, 0}, {4, 3073}, {4, 0}}, "frame_grid of no keys");
    ok &= check({{28, 1}, {4, 3073}, {4, 1}, {16, 1}, {4, 2}, {4, 0}}, "features_in_area, no capacity");
    ok &= check({{16, 3649}, {12, 3649}, {4, 3649}, {4, 3649}, {1, 3649}, {4, 7}, {8, 33}}, "local map, odd entries");
    ok &= check({{16, 0}, {12, 0}, {4, 0}, {4, 0}, {1, 0}, {4, 0}, {8, 0}, {2, 0}}, "eight empty regions");
    // pseudo-random lists of one to eight regions
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st >> 12; st ^= st << 25; st ^= st >> 27; return (st * 0x2545F4914F6CDD1Dull) >> 33; };
    for (int l = 0; l < 40; ++l) {
        std::vector<Req> list(1 + next() % olf::kCarveMaxRegions);
        for (Req& r : list) r = {elems[next() % 7], counts[next() % 7]};
        ok &= check(list, "random");
    }
    // more than 4 GB in all: the offsets are size_t throughout
    {
        const std::vector<Req> big = {{16, 200000001}, {2, 3}, {4, 300000001}, {28, 0}, {12, 7}};
        olf::CarveLayout k;
        void* p[5];
        for (size_t i = 0; i < big.size(); ++i) add(k, big[i].elem, &p[i], big[i].count);
        if (k.total() <= ((size_t)1 << 32)) { std::printf("FAIL big: total %zu does not exceed 4 GB\n", k.total()); ok = false; }
        ok &= check(big, "more than 4 GB");
    }
    std::printf("%s %d lists\n", ok ? "STAGING_LAYOUT_OK" : "STAGING_LAYOUT_FAILED", g_lists);
    return ok ? 0 : 1;
}
