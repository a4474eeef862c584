// uvs_solve_dstep256.hip -- k_solve_dstep (uvs_solve_kernel.h: the persistent LM kernel's debug-step instantiation behind uvs_debug_step) with 256 threads
// per workgroup, the build of the 256-thread k_solve in uvs_solver.hip.  Its own translation unit so that the product kernel's register figures stay those of
// a module without it (the two would share the noinline factorization calls).  The namespace is renamed as in uvs_solve512.hip.
#define UVS_EMIT_K_SOLVE_DSTEP 1
#define uvsdev uvsdev256d
#include "uvs_solve_kernel.h"

using namespace uvsdev256d;

extern "C" {
// block table of the output-stationary gather (this translation unit's __constant__ copies) + the LDS opt-in; once per device
int uvs_k_solve256d_init(const unsigned char* fa, const unsigned char* fb, int n) {
    return unit_init(fa, fb, n, {(const void*)k_solve_dstep});
}
// kopts / ds: the caller's uvsdev::KOpts / uvsdev::DebugStep (same definitions, other namespace); window 0 of the uploaded batch
int uvs_k_solve256d_launch(hipStream_t stream, char* blobs, const long long* blob_off, double* ws_all, const long long* ws_off,
                           const void* kopts, size_t kopts_bytes, uvs_report* reports, const void* ds, size_t ds_bytes) {
    KOpts ko; DebugStep d;
    if (kopts_bytes != sizeof(ko) || ds_bytes != sizeof(d)) return UVS_ERR_INVALID_ARG;
    __builtin_memcpy(&ko, kopts, sizeof(ko)); __builtin_memcpy(&d, ds, sizeof(d));
    hipLaunchKernelGGL(k_solve_dstep, dim3(1), dim3(NT), LDS_BYTES, stream, blobs, blob_off, ws_all, ws_off, ko, reports, d);
    return UVS_OK;
}
}
