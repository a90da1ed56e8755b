// profiles/topic_records_host_loops.cpp — what a caller does on the host today for prefiltering/colored_points: the message is unpacked a second time
// (pcl::fromROSMsg: one field copy per point into the 32-byte pcl::PointXYZI) and the loop of apps/prefiltering_component.cpp:240-253 fills a
// pcl::PointXYZRGB cloud, which pcl::toROSMsg then copies as it is (that copy is NOT included: the baseline is the cheaper for it).  The 32-byte loop of
// the aligned and keyframe clouds is profiles/scan_egress_host_loop.cpp.  Built -O2 into a small shared object by profiles/topic_records_profile.py.
#include <cstddef>
#include <cstdint>
#include <cstring>

struct alignas(16) PointXYZI {
    float x, y, z, w;  // data[3] = 1.0f
    float intensity, pad[3];
};
struct alignas(16) PointXYZRGB {
    float   x, y, z, w;
    uint8_t b, g, r, a;
    float   pad[3];
};
static_assert(sizeof(PointXYZI) == 32 && sizeof(PointXYZRGB) == 32, "the PCL points in memory");

extern "C" void unpack_xyzi(const uint8_t* data, std::size_t n, std::size_t point_step, std::size_t ox, std::size_t oy, std::size_t oz, std::size_t oi, PointXYZI* out)
{
    const PointXYZI blank{0.0f, 0.0f, 0.0f, 1.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    for (std::size_t i = 0; i < n; ++i) out[i] = blank;  // cloud.points.resize(n)
    for (std::size_t i = 0; i < n; ++i) {
        const uint8_t* p = data + i * point_step;
        std::memcpy(&out[i].x, p + ox, 4);
        std::memcpy(&out[i].y, p + oy, 4);
        std::memcpy(&out[i].z, p + oz, 4);
        std::memcpy(&out[i].intensity, p + oi, 4);
    }
}

extern "C" void colour_loop(const PointXYZI* cloud, std::size_t n, PointXYZRGB* out)
{
    const PointXYZRGB blank{0.0f, 0.0f, 0.0f, 1.0f, 0, 0, 0, 255, {0.0f, 0.0f, 0.0f}};
    for (std::size_t i = 0; i < n; ++i) out[i] = blank;  // colored->resize(cloud->size())
    for (int i = 0; i < (int)n; i++) {                   // :247-253
        double t = static_cast<double>(i) / n;
        std::memcpy(&out[i].x, &cloud[i].x, 16);         // getVector4fMap() = getVector4fMap()
        out[i].r = 255 * t;
        out[i].g = 128;
        out[i].b = 255 * (1 - t);
    }
}
