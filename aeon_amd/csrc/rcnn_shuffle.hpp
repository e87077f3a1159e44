// rcnn_shuffle.hpp -- std::shuffle over std::minstd_rand0 as libstdc++ (GCC 11) performs it, in plain
// 32-bit integer C++ that compiles for the host and for the device.
//
// localization::rcnn::transformer::sample_anchors (etl_localization_rcnn.cpp:222-261) shuffles its
// foreground and background lists with std::shuffle and the record's engine and keeps a prefix of
// each.  Which permutation std::shuffle produces is the library's choice, not the standard's; this
// restates bits/stl_algo.h (shuffle, __gen_two_uniform_ints) and bits/uniform_int_dist.h
// (uniform_int_distribution<size_t>::operator(), the "downscaling" branch) of libstdc++ 11:
//   * while urng_range / n >= n (n <= 46340 for minstd_rand0), two swap positions come from one draw
//     over [0, i * (i + 1)), after a single leading swap from a draw over [0, 1] when n is even;
//   * above that, one draw over [0, i] per swap;
//   * a draw over [0, b]: scaling = range / (b + 1), past = (b + 1) * scaling, the engine is drawn
//     until value - min < past, the result is that / scaling.
// Every quantity is below 2^31 (range = 2^31 - 3, n < 2^31), so the library's 64-bit arithmetic is done
// in 32 bits here with the same results.  tests/test_rcnn.py compares this header, compiled for the
// host, with the real std::shuffle (permutation and engine end state).
//
// A permutation depends on n alone, so the shuffle runs over ranks 0..n-1.  Only a prefix of the result
// is used: swap i exchanges position i -- still holding rank i, as no earlier swap reached it -- with
// a position j <= i, so positions below `keep` only ever receive the value i from a swap i >= keep, and
// the prefix is computed with `keep` words of storage however large n is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RCNN_HD __host__ __device__
#else
#define RCNN_HD
#endif

namespace aeon_hip {

// std::minstd_rand0: x <- 16807 x mod (2^31 - 1); min 1, max 2^31 - 2
struct minstd0 {
    uint32_t x;
    RCNN_HD uint32_t next()
    {
        const uint64_t p = (uint64_t)x * 16807u;
        uint32_t       r = (uint32_t)(p & 0x7fffffffu) + (uint32_t)(p >> 31);
        if (r >= 0x7fffffffu) r -= 0x7fffffffu;
        return x = r;
    }
};
// an engine word as minstd_rand0::seed takes it: mod 2^31 - 1, and 0 becomes 1 (the LCG never leaves 0,
// and a draw of 0 would be refused by rcnn_uniform's loop for ever)
RCNN_HD inline uint32_t rcnn_engine_word(uint32_t s) { return s % 2147483647u == 0 ? 1u : s % 2147483647u; }
constexpr uint32_t kRcnnUrngRange = 2147483646u - 1u; // max() - min()

// uniform_int_distribution<size_t>{0, b}(g), b < kRcnnUrngRange
RCNN_HD inline uint32_t rcnn_uniform(minstd0& g, uint32_t b)
{
    const uint32_t uerange = b + 1;
    const uint32_t scaling = kRcnnUrngRange / uerange;
    const uint32_t past    = uerange * scaling;
    uint32_t       ret;
    do ret = g.next() - 1u;
    while (ret >= past);
    return ret / scaling;
}

// swap(position i, position j), j <= i, restricted to the kept prefix out[0 .. m)
RCNN_HD inline void rcnn_prefix_swap(int32_t* out, uint32_t m, uint32_t i, uint32_t j)
{
    if (i < m) {
        const int32_t t = out[i];
        out[i]          = out[j];
        out[j]          = t;
    } else if (j < m) {
        out[j] = (int32_t)i;
    }
}

// whether std::shuffle over n elements draws two swap positions at once
RCNN_HD inline bool rcnn_shuffle_pairs(uint32_t n) { return kRcnnUrngRange / n >= n; }

// the first min(n, keep) entries of std::shuffle(iota(0, n), g) into out; g advances as for the whole
// shuffle.  n - 1 must be below kRcnnUrngRange.
RCNN_HD inline void rcnn_shuffle_prefix(uint32_t n, uint32_t keep, minstd0& g, int32_t* out)
{
    const uint32_t m = n < keep ? n : keep;
    for (uint32_t i = 0; i < m; i++) out[i] = (int32_t)i;
    if (n < 2) return;
    auto swap_ij = [&](uint32_t i, uint32_t j) { rcnn_prefix_swap(out, m, i, j); };
    if (rcnn_shuffle_pairs(n)) {
        uint32_t i = 1;
        if ((n & 1u) == 0) {
            swap_ij(i, rcnn_uniform(g, 1));
            i++;
        }
        while (i != n) {
            const uint32_t b0 = i + 1, b1 = i + 2;
            const uint32_t x = rcnn_uniform(g, b0 * b1 - 1);
            swap_ij(i, x / b1);
            swap_ij(i + 1, x % b1);
            i += 2;
        }
        return;
    }
    for (uint32_t i = 1; i != n; i++) swap_ij(i, rcnn_uniform(g, i));
}

} // namespace aeon_hip
