// profiles/scan_egress_host_loop.cpp — what a caller of mrgfe_scan_callback does on the host to get the message's records: the per-point loop of
// include/mrgfe_pcl_filters.hpp detail::unpack (assign(n, PointT()), then four stores per point) into the 32-byte pcl::PointXYZI, which pcl::toROSMsg then
// copies as it is.  Built -O2 into a small shared object by profiles/scan_egress_profile.py; the copy toROSMsg makes is NOT included (the baseline is the
// cheaper for it).
#include <cstddef>

struct alignas(16) PointXYZI {
    float x, y, z, w;  // data[3] = 1.0f
    float intensity, pad[3];
};
static_assert(sizeof(PointXYZI) == 32, "pcl::PointXYZI in memory");

extern "C" void records_from_packed(const float* xyzi, std::size_t n, PointXYZI* out)
{
    const PointXYZI blank{0.0f, 0.0f, 0.0f, 1.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    for (std::size_t i = 0; i < n; ++i) out[i] = blank;  // output.points.assign(n, PointT())
    for (std::size_t i = 0; i < n; ++i) {
        PointXYZI& p = out[i];
        p.x = xyzi[4 * i];
        p.y = xyzi[4 * i + 1];
        p.z = xyzi[4 * i + 2];
        p.intensity = xyzi[4 * i + 3];
    }
}
