// uvs_handle.h -- the host scaffolding the front-end units share, one statement of each: what every handle owns besides its buffers (device,
// stream, timing events, error text) with the way it is opened and closed, and the sizes and the bump arena of the packed call buffers.
// Used by uvs_pose_graph, uvs_loop_verify, uvs_vanishing_points, uvs_keyframe_features and, through uvs_ft_handle.h, the
// three units of the point front end.  Nothing here runs on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/uvs_solver.h"
#include "uvs_hip_buf.h"

inline size_t align_up(size_t b, size_t a) { return (b + a - 1) / a * a; }
inline int pitch_of(int width) { return (width + 15) & ~15; }      // bytes of an image row: every row starts 16-byte aligned

// byte offsets in one buffer, each a multiple of 256; `o` is the bytes taken so far
struct UvsArena {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; }
};

// Base of every handle struct.  A *_create makes the handle with new, calls open(), allocates; on a failure, and in *_destroy, it calls close()
// and deletes the handle.  The buffers of the derived struct are freed before the stream is destroyed.
struct UvsHandle {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;    // around the device work of one call (the *_last_*device_ms calls); null in a handle that times nothing
    std::string err;
    ~UvsHandle() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (st) (void)hipStreamDestroy(st);
    }
    int open(int dev, bool timed = true) {
        device = dev;
        hipError_t e;
        if ((e = hipSetDevice(dev)) != hipSuccess) return hip_fail(err, e, "hipSetDevice");
        if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) return hip_fail(err, e, "hipStreamCreate");
        if (timed && ((e = hipEventCreate(&ev0)) != hipSuccess || (e = hipEventCreate(&ev1)) != hipSuccess)) return hip_fail(err, e, "hipEventCreate");
        return UVS_OK;
    }
    void close() {                              // the device work in flight ends before the caller deletes the handle
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
    }
};
