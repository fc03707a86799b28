// refsum.h - torch.sum(x + add, -1) of a contiguous fp32 row in the order torch's CPU kernel evaluates it (x86 hosts).
//
// The reference normalises its pdf by torch.sum(weights + 1e-5, -1) (utils.py:200-201) on the CPU.  That sum is ATen's
// cascade sum (aten/src/ATen/native/cpu/SumKernel.cpp) with fp32 accumulators over 8-lane vectors: the same order under
// ATEN_CPU_CAPABILITY default, avx2 and avx512 (the sum kernel has no 16-lane variant).  This header restates that order
// as scalar code, one correctly rounded fp32 add at a time and no reassociation, for the host entry
// (snerf_reference_sum_host_f32) and, lane by lane, for the device (sampler.hip).  tests/test_reference_sum_order.py holds it
// against torch bit for bit.
//
// The order, for x'[i] = fl(x[i] + add), V = 8 lanes, ILP = 4 columns, 4 cascade levels:
//   n < V:   row_sum over scalars - column k takes x'[4r + k] for r < n/4; the rest go into column 0 in order;
//            then col0 += col1, += col2, += col3.
//   n >= V:  nv = n/8 vectors; every vector lane l runs row_sum over x'[8v + l] (column k takes vector 4r + k through the
//            level cascade, leftover vectors 4*(nv/4) .. nv-1 go into column 0, then the columns fold into column 0);
//            finally fin = 0, += the scalar tail x'[8nv .. n) in order, += the 8 lane partials, lane 0 first.
//   cascade: level_step = 1 << max(4, ceil_log2(rows)/4); after each full block of level_step rows acc1 += acc0, acc0 = 0,
//            and further up while the row counter is a multiple of the next level's span; the rows after the last full
//            block go into level 0; then acc0 += acc1, += acc2, += acc3.
// Rows of 32768 elements and more may be split over threads by torch: out of scope (the entries take n <= 32767).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SNERF_REFSUM_HD __host__ __device__
#else
#define SNERF_REFSUM_HD
#endif

namespace snerf {
namespace refsum {

constexpr int V = 8;        // lanes of ATen's Vectorized<float> on x86 (default, AVX2; the sum kernel has no AVX-512 form)
constexpr int ILP = 4;      // row_sum's columns (ilp_factor)
constexpr int MAX_N = 32767;

// one correctly rounded fp32 add, never contracted or reassociated
SNERF_REFSUM_HD inline float add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

// ATen's utils::CeilLog2
SNERF_REFSUM_HD inline int ceil_log2(int64_t x) {
    if (x <= 2) return 1;
    uint64_t v = (uint64_t)x - 1;
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// multi_row_sum's level cascade for one column of `rows` values get(0), get(1), ...
template <class Get>
SNERF_REFSUM_HD inline float cascade(const Get &get, int64_t rows) {
    const int lp0 = ceil_log2(rows) / 4;
    const int power = lp0 > 4 ? lp0 : 4;
    const int64_t step = (int64_t)1 << power, mask = step - 1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t i = 0;
    while (i + step <= rows) {
        for (int64_t j = 0; j < step; ++j, ++i) a0 = add(a0, get(i));
        a1 = add(a1, a0), a0 = 0.f;
        if ((i & (mask << power)) != 0) continue;
        a2 = add(a2, a1), a1 = 0.f;
        if ((i & (mask << (2 * power))) != 0) continue;
        a3 = add(a3, a2), a2 = 0.f;
    }
    for (; i < rows; ++i) a0 = add(a0, get(i));
    a0 = add(a0, a1);
    a0 = add(a0, a2);
    return add(a0, a3);
}

// row_sum of ATen for a stream of n values at(0) .. at(n-1) (scalars, or one lane of the vectors)
template <class At>
SNERF_REFSUM_HD inline float row_sum(const At &at, int64_t n) {
    const int64_t rows = n / ILP;
    float c[ILP];
    for (int k = 0; k < ILP; ++k) c[k] = cascade([&](int64_t r) { return at(ILP * r + k); }, rows);
    for (int64_t t = ILP * rows; t < n; ++t) c[0] = add(c[0], at(t));
    for (int k = 1; k < ILP; ++k) c[0] = add(c[0], c[k]);
    return c[0];
}

// the whole row: torch.sum(x[0 .. n) + a) as torch's CPU kernel returns it
SNERF_REFSUM_HD inline float row(const float *x, int64_t n, float a) {
    if (n < V) return row_sum([&](int64_t i) { return add(x[i], a); }, n);
    const int64_t nv = n / V;
    float fin = 0.f;
    for (int64_t j = V * nv; j < n; ++j) fin = add(fin, add(x[j], a));
    for (int l = 0; l < V; ++l) fin = add(fin, row_sum([&](int64_t v) { return add(x[V * v + l], a); }, nv));
    return fin;
}

}  // namespace refsum
}  // namespace snerf
