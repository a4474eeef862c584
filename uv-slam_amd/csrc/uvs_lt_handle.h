// uvs_lt_handle.h -- the handle behind the uvs_lt_* calls, shared by the three units of the line front end: csrc/uvs_line_track.hip (creates and
// destroys it, describes and matches segments, keeps the slots' previous lines), csrc/uvs_line_detect.hip (detects the segments of an image
// and hands them to the tracking unit without a second upload of the image) and csrc/uvs_line_undistort.hip (the slots' undistortion maps and
// the remap of a raw image, which the detection unit calls in front of its own kernels).  Device, stream, events and error text are the base's
// (uvs_handle.h).  Host only, but for the three structs the kernels read.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_handle.h"

namespace uvslt {

constexpr int kRows = UVS_LT_ROWS, kFloats = UVS_LT_DESC_FLOATS, kBytes = UVS_LT_DESC_BYTES;
constexpr int kMaxLines = UVS_LT_MAX_LINES;

struct LtItem {                    // device copy of one item
    int W, H, n_lines, l_off;      // image size; lines, offset of the first one in the concatenated arrays
    long long img_off;             // of the image in the packed input
    uint8_t* slot_desc;            // where the new lines' descriptors [n][32], gate points [n][4] and statuses [n] go (the slot's new set)
    int32_t* slot_ends;
    int32_t* slot_stat;
};
struct LtMatchJob {                // one match: the queries, the train set, the outputs (each may be null)
    const uint8_t* pdesc; const int32_t* pends; const int32_t* pstat;      // pstat / cstat null: every line is OK
    const uint8_t* cdesc; const int32_t* cends; const int32_t* cstat;
    int n_prev, n_cur;
    int32_t* match_of_prev; int32_t* dist_prev; int32_t* prev_of_cur; int32_t* dist_cur;
    uvs_lt_result* result;         // n_matched is written here
};
struct UdItem {                    // one remap: the raw image W x H at src_off, n_out = Wo Ho output pixels at dst_off, the slot's map [n_out][2]
    int W, H, n_out, pad;
    long long src_off, dst_off;
    const int32_t* map;
};

}  // namespace uvslt

struct LtSlot { int n_prev = 0, cur = 0; };      // lines of the previous set; which of the slot's two sets holds it
// a slot's undistortion (uvs_line_undistort.hip): the raw size W x H, the output size Wo x Ho, the map [Ho][Wo][2] in Q5.  uvs_lt_reset keeps it
struct LtUndistort { bool on = false; int W = 0, H = 0, Wo = 0, Ho = 0; DevBuf<int32_t> map; };

struct uvs_lt_tracker : UvsHandle {
    int max_streams = 0, max_width = 0, max_height = 0, max_lines = 0, max_length = 0;
    float device_ms = 0.f;                      // uvs_lt_last_device_ms
    size_t in_bytes = 0, out_bytes = 0, grad_stride = 0;
    std::vector<LtSlot> slots;
    DevBuf<char> d_in, d_out;                   // packed inputs (items | jobs | segments | images) / outputs of one call
    PinnedBuf<char> h_in, h_out;                // pinned staging
    DevBuf<uint32_t> d_grad;                    // [items][max_width max_height] gx | gy
    DevBuf<int32_t> d_geom, d_line_item;        // [lines][8]; [lines]
    DevBuf<long long> d_S;                      // [lines][63][4]
    DevBuf<double> d_tables;                    // G[63] | Lc[21]
    DevBuf<uint8_t> d_slot_desc;                // [streams + 1][2][max_lines][32]: the slots' two sets; the last "slot" is the debug call's
    DevBuf<int32_t> d_slot_ends, d_slot_stat;   // [streams + 1][2][max_lines][4]; [streams + 1][2][max_lines]
    DevBuf<double> d_dbg_float;                 // uvs_lt_debug_line only: [72]
    // detection (uvs_line_detect.hip): allocated by the first call that needs them, so that a tracker that never detects pays nothing.
    // px = max_width max_height, per item of a call (at most max_streams)
    float detect_ms = 0.f;                      // uvs_lt_last_detect_device_ms
    PinnedBuf<char> h_det_in, h_det_out;        // pinned staging: (items | images) / (results | seg | width2 | info)
    DevBuf<char> d_det_in, d_det_out;
    DevBuf<uint8_t> d_det_blur, d_det_sec, d_det_vote;      // [items][px]; [items][2][px] sector A, sector B; [items][px]
    DevBuf<uint32_t> d_det_grad;                // [items][px] gx | gy of the blurred image
    DevBuf<int32_t> d_det_label;                // [items][2][px]: the union-find parents, then the regions' names
    DevBuf<char> d_det_rec;                     // [items][2][px] records of 64 bytes, read at a region's name only
    DevBuf<unsigned long long> d_det_list_len;  // [items][px] the kept segments in no order: the bits of the length ...
    DevBuf<uint32_t> d_det_list_id;             // ... and 2 name + partition
    // undistortion (uvs_line_undistort.hip): a slot's map is allocated by its first set call, the staging by the first uvs_lt_undistort
    float undistort_ms = 0.f;                   // uvs_lt_last_undistort_device_ms
    std::vector<LtUndistort> ud;                // [max_streams]
    PinnedBuf<char> h_ud_io;                    // uvs_lt_undistort's pinned staging and device buffer, one layout: (items | raw images | outputs)
    DevBuf<char> d_ud_io;

    uint8_t* set_desc(int slot, int set) const { return d_slot_desc + ((size_t)(2 * slot + set) * max_lines) * uvslt::kBytes; }
    int32_t* set_ends(int slot, int set) const { return d_slot_ends + ((size_t)(2 * slot + set) * max_lines) * 4; }
    int32_t* set_stat(int slot, int set) const { return d_slot_stat + (size_t)(2 * slot + set) * max_lines; }
};

namespace uvslt {

struct LtLayout { size_t o_jobs, o_seg, o_img, in_used, o_desc, o_stat, o_prev, o_dist, out_used; };

// offsets of one call's packed buffers for n items, tl lines and the given image bytes (each image starts 256-aligned)
inline LtLayout lt_layout(size_t n, size_t tl, const std::vector<size_t>& img_bytes, std::vector<size_t>* img_off) {
    LtLayout Y;
    UvsArena in;
    (void)in.take(n * sizeof(LtItem));
    Y.o_jobs = in.take(n * sizeof(LtMatchJob));
    Y.o_seg = in.take(tl * 32);
    Y.o_img = in.o;
    for (size_t b : img_bytes) { const size_t at = in.take(b); if (img_off) img_off->push_back(at); }
    Y.in_used = in.o;
    UvsArena out;
    (void)out.take(n * sizeof(uvs_lt_result));
    Y.o_desc = out.take(tl * kBytes); Y.o_stat = out.take(tl * 4); Y.o_prev = out.take(tl * 4); Y.o_dist = out.take(tl * 4);
    Y.out_used = out.o;
    return Y;
}

inline int lt_check_items(uvs_lt_tracker* h, const std::string& fn, int n_items, const uvs_lt_item* items, bool slots, size_t* tl_out, int* max_n_out) {
    std::vector<char> seen(h->max_streams, 0);
    size_t tl = 0; int max_n = 0;
    for (int b = 0; b < n_items; ++b) {
        const uvs_lt_item& it = items[b];
        const std::string who = fn + ": item " + std::to_string(b);
        if (!it.image || it.n_lines < 0 || (it.n_lines > 0 && !it.segments)) { h->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
        if (slots) {
            if (it.stream < 0 || it.stream >= h->max_streams) { h->err = who + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
            if (seen[it.stream]) { h->err = who + ": stream given twice"; return UVS_ERR_INVALID_ARG; }
            seen[it.stream] = 1;
        }
        if (it.width < UVS_LT_MIN_SIZE || it.height < UVS_LT_MIN_SIZE) { h->err = who + ": width or height below UVS_LT_MIN_SIZE"; return UVS_ERR_INVALID_ARG; }
        if (it.width > h->max_width || it.height > h->max_height || it.n_lines > h->max_lines) {
            h->err = who + " exceeds the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY;
        }
        for (int l = 0; l < it.n_lines; ++l)
            for (int k = 0; k < 4; ++k) {
                const double v = it.segments[4 * (size_t)l + k];
                if (!std::isfinite(v) || std::fabs(v) > UVS_KF_MAX_COORD) { h->err = who + ": a coordinate is not finite or beyond UVS_KF_MAX_COORD"; return UVS_ERR_INVALID_ARG; }
            }
        tl += it.n_lines; max_n = std::max(max_n, it.n_lines);
    }
    *tl_out = tl; *max_n_out = max_n;
    return UVS_OK;
}

// One call's device work of the tracking unit (uvs_line_track.hip), through the download and the wait.  slot_of[b]: the slot whose sets item b
// uses (max_streams = the debug call's); with `match`, the slot's previous set is matched against the new one.  The caller swaps the slots'
// sets after a success.  dev_images: null, or device memory that already holds the items' images at dev_img_off[b] (uvs_lt_detect_track: the
// images are not uploaded a second time).
int lt_run(uvs_lt_tracker* h, int n_items, const uvs_lt_item* items, const std::vector<int>& slot_of, bool match, size_t tl, int max_n,
           double* dbg_float, LtLayout* layout, const uint8_t* dev_images = nullptr, const size_t* dev_img_off = nullptr);

// The remap kernel of uvs_line_undistort.hip on the handle's stream: n items (the device array `items`) of at most max_out output pixels, the raw
// images at src + src_off, the outputs at dst + dst_off.  uvs_lt_detect_track launches it between its upload and its first kernel.
int ud_launch(uvs_lt_tracker* h, int n, const UdItem* items, const uint8_t* src, uint8_t* dst, int max_out);

}  // namespace uvslt
