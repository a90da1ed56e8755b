// csrc/sor_threshold.h — pcl::StatisticalOutlierRemoval's threshold (pcl/filters/impl/statistical_outlier_removal.hpp, reached from
// apps/prefiltering_component.cpp:189-192) as ONE piece of host/device code.
//
// The reference adds, point after point in f64,  sum += dist_i,  sq_sum += float(dist_i * dist_i)  and counts the points whose k neighbours were
// all found; then  mean = sum / valid,  variance = (sq_sum - sum^2 / valid) / (valid - 1),  thr = mean + mul * sqrt(variance).  The same source runs
//   * on the HOST: the sequential loop of filter_statistical_outlier_device (the host-driven prefilter), the re-check of a device threshold,
//     and the diagnostic mrgfe_dbg_sor_threshold;
//   * on the DEVICE inside sor_reduce_tiles_kernel / sor_finish_kernel (filters.hip), which add the terms in a TREE and certify that the order
//     did not matter.
// The certificate.  All terms are non-negative floats.  Let 2^q be the lowest set bit over all non-zero terms: every term, and so every partial
// sum in every order, is a multiple of 2^q.  If the tree sum is below 2^(q + 52), every partial sum in every order is a multiple of 2^q below
// 2^53 * 2^q, hence representable: no addition rounded, and the sequential sum has the same bits.  (The bound is one bit tighter than the
// argument needs, which covers a tree sum that was itself rounded: a rounded sum is at least 2^(q + 53).)  A negative or non-finite term is
// never certified.  All arithmetic in the written order: compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#ifndef MRGFE_HD
#define MRGFE_HD __host__ __device__ inline
#endif

namespace mrgfe {
namespace sor {

constexpr int32_t kNoTerm = 0x7fffffff;     // lowest-bit exponent of "no non-zero term yet": the neutral element of the minimum
constexpr int32_t kBadTerm = -0x7fffffff;   // a negative or non-finite term: below every bound, the certificate fails

// q with 2^q = the lowest set bit of a non-negative finite float; kNoTerm for +-0, kBadTerm for a negative or non-finite value
MRGFE_HD int32_t low_bit_exponent(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    if ((b & 0x7fffffffu) == 0u) return kNoTerm;
    const uint32_t e = (b >> 23) & 0xffu;
    if ((b >> 31) != 0u || e == 0xffu) return kBadTerm;
    uint32_t m = b & 0x7fffffu;
    int32_t  q = -149;  // subnormal: m * 2^-149
    if (e != 0u) { m |= 0x800000u; q = static_cast<int32_t>(e) - 150; }
    return q + __builtin_ctz(m);  // (m != 0)
}

MRGFE_HD int32_t min_exponent(int32_t a, int32_t b) { return b < a ? b : a; }

// the two terms a point contributes
MRGFE_HD float square_term(float dist)
{
    const float d2 = dist * dist;  // a float product, as in the reference
    return d2;
}

// does a sum of non-negative terms whose lowest set bits are >= 2^q, added in SOME order with the result `tree_sum`, have the same bits in every order?
MRGFE_HD bool certified(double tree_sum, int32_t q)
{
    if (q == kNoTerm) return true;  // every term is zero
    if (q == kBadTerm || !(tree_sum >= 0.0)) return false;
    // 2^(q + 52): q is in [-149, 127], a normal double
    const uint64_t bits = static_cast<uint64_t>(q + 52 + 1023) << 52;
    double         bound;
    memcpy(&bound, &bits, 8);
    return tree_sum < bound;
}

// mean / variance / threshold from the sums (the reference's expressions, f64)
MRGFE_HD double threshold(double sum, double sq_sum, uint64_t valid, double stddev_mul)
{
    const double nv = static_cast<double>(valid);
    const double mean = sum / nv;
    const double variance = (sq_sum - sum * sum / nv) / (nv - 1);
    return mean + stddev_mul * sqrt(variance);
}

MRGFE_HD bool same_bits(double a, double b)
{
    if (a != a && b != b) return true;  // two NaNs count as equal
    uint64_t x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x == y;
}

// What a reduction reports: the two sums, the count, the lowest-bit exponents of the terms of either sum, the threshold and whether both sums
// are certified to be the sequential ones.
struct Result {
    double   sum, sq_sum, thr;
    uint64_t valid;
    int32_t  q_sum, q_sq;
    uint32_t certified, pad;
};

// the reference's loop itself (host).  kWithCertificate: the exponents and the certificate of its own sums ride along (the diagnostic, the tests); without,
// the loop is the reference's and nothing else (the host-driven prefilter pass, which needs the threshold only) and `certified` stays 0
template <bool kWithCertificate = true>
inline Result sequential(const float* dist, const uint32_t* valid, size_t n, double stddev_mul)
{
    Result r;
    memset(&r, 0, sizeof(r));
    r.q_sum = r.q_sq = kNoTerm;
    for (size_t i = 0; i < n; ++i) {
        const float d2 = square_term(dist[i]);
        r.sum += dist[i];
        r.sq_sum += d2;
        r.valid += valid[i];
        if (kWithCertificate) {
            r.q_sum = min_exponent(r.q_sum, low_bit_exponent(dist[i]));
            r.q_sq = min_exponent(r.q_sq, low_bit_exponent(d2));
        }
    }
    r.thr = threshold(r.sum, r.sq_sum, r.valid, stddev_mul);
    if (kWithCertificate) r.certified = (certified(r.sum, r.q_sum) && certified(r.sq_sum, r.q_sq)) ? 1u : 0u;
    return r;
}

}  // namespace sor
}  // namespace mrgfe
