// csrc/ingest.h — point-layout ingest (ingest.hip): strided point records -> packed float4 on the device.
#pragma once
#include "common.h"

namespace mrgfe {

int launch_gather_points(mrgfe_ctx* ctx, const void* d_raw, float4* d_dst, size_t n, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz,
                         int32_t oi);
// raw record bytes -> the context's raw buffer (*d_raw), one stream-ordered copy through the pinned staging ring
int upload_raw_records(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, const void** d_raw);
// the same copy to a place of the caller's (several messages behind one another in one device buffer: each takes the ring's next slot)
int upload_raw_records_to(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, void* d_dst);
// MRGFE_OK, or MRGFE_ERR_INVALID with the message set; a row_step of 0 becomes width * point_step.  `ctx`: the context the call runs on — with its
// mrgfe_ctx_set_byte_layouts switch on, offsets and steps need not be multiples of 4 and fields may overlap
int check_pointcloud2_layout(const mrgfe_ctx* ctx, const char* fn, uint32_t width, uint32_t height, uint32_t point_step, uint32_t* row_step, uint32_t off_x, uint32_t off_y,
                             uint32_t off_z, int32_t off_intensity);
// what the rules demand with the switch off (row_step filled in): such a layout is read by the strict kernel instantiations (scan_point.h
// load_point_record), whatever the switch says; every other layout by their byte-aligned twins (load_point_record_bytes)
inline bool layout_is_strict(uint32_t point_step, uint32_t row_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, int32_t off_intensity)
{
    return ((point_step | row_step | off_x | off_y | off_z | (off_intensity >= 0 ? static_cast<uint32_t>(off_intensity) : 0u)) & 3u) == 0;
}
int upload_gathered(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, size_t n, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz,
                    int32_t oi, void* d_dst);

}  // namespace mrgfe
