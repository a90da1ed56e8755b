// csrc/record_store.h — the wire record of one point, the one text of the two layouts the egress calls write (mapcloud.hip: mrgfe_map_store_publish / _read;
// filters.hip: mrgfe_scan_callback_records, mrgfe_prefilter_records, mrgfe_cloud_records_device):
//   point_step 32: x, y, z, 1.0f | intensity, 0, 0, 0   the pcl::PointXYZI in memory, which is what pcl::toROSMsg copies (two 16-byte stores)
//   point_step 16: x, y, z, intensity                   the body of a binary PCD (one 16-byte store)
// Per point: up to two f32 offset additions per coordinate, one after the other (the save offsets of the map), then the stores.  Without offsets no
// arithmetic touches the point: its bits, a NaN's payload included, are those of the kernel that made it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mrgfe {

struct EgressOffsets { int32_t n; float v[2][3]; };
template <int kStep>
__device__ __forceinline__ void store_record(float4* __restrict__ out, size_t at, float4 p, const EgressOffsets& o)
{
#pragma clang fp contract(off)
    for (int k = 0; k < o.n; ++k) {
        p.x = p.x + o.v[k][0];
        p.y = p.y + o.v[k][1];
        p.z = p.z + o.v[k][2];
    }
    if (kStep == 16) out[at] = p;
    else {
        out[2 * at] = make_float4(p.x, p.y, p.z, 1.0f);
        out[2 * at + 1] = make_float4(p.w, 0.0f, 0.0f, 0.0f);
    }
}

}  // namespace mrgfe
