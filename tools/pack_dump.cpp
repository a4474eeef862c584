// pack_dump.cpp -- packs one window file (UVSWIN01: host/window_io.h, abi.Window.save) with the host-only packing unit and writes the blob.
// No HIP anywhere: the program of tests/test_pack_blob.py (blob digests, header integers, rejections) and of sanitizer runs of the packing:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/pack_dump.cpp uv-slam_amd/csrc/uvs_pack.cpp -o pack_dump -pthread
//   pack_dump <window> <blob out> [td] [ex] [all] [dst] [grid=<chunk_grid>] [cache=<window packed first through the same PackCache>]
// stdout: "ok <the twelve integers of uvs_debug_pack_layout> <out_host> <cur_sel> <cache hit> <placed through PackDst>", or "error <status> <text>";
// the exit status is 0 for both (a rejection is a result), 2 for a file that does not load.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../uv-slam_amd/csrc/uvs_pack.h"
#include "../uv-slam_amd/host/window_io.h"
using namespace uvspack;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: pack_dump <window> <blob out> [td] [ex] [all] [dst] [grid=N] [cache=<window>]\n"); return 2; }
    uvs_options o; std::memset(&o, 0, sizeof(o));      // the packing reads estimate_td and estimate_extrinsic only
    int grid = 0; bool all_blocks = false, use_dst = false; std::string first;
    for (int a = 3; a < argc; ++a) {
        const std::string s = argv[a];
        if (s == "td") o.estimate_td = 1; else if (s == "ex") o.estimate_extrinsic = 1; else if (s == "all") all_blocks = true; else if (s == "dst") use_dst = true;
        else if (s.rfind("grid=", 0) == 0) grid = std::atoi(s.c_str() + 5); else if (s.rfind("cache=", 0) == 0) first = s.substr(6);
        else { std::fprintf(stderr, "unknown switch %s\n", s.c_str()); return 2; }
    }
    WindowFile wf, wf0;
    if (!wf.load(argv[1]) || (!first.empty() && !wf0.load(first))) { std::fprintf(stderr, "cannot load the window file\n"); return 2; }
    std::vector<char> out; DevWin h; std::string err; PackCache cache; bool hit = false;
    if (!first.empty()) {
        const int rc0 = pack_window(&wf0.w, o, out, h, err, grid, &cache, nullptr, all_blocks);
        if (rc0 != UVS_OK) { std::printf("error %d %s\n", rc0, err.c_str()); return 0; }
        hit = cache.matches(&wf.w, o, grid, all_blocks) && out.size() == (size_t)cache.hdr.blob_bytes;
    }
    // PackDst: a heap buffer stands in for the pinned staging buffer, filled with a pattern (the packing must write every byte of its blob) and
    // entered at an offset (a multiple of 256 bytes, as a batch's earlier windows leave it)
    std::vector<char> heap(use_dst ? (size_t)64 << 20 : 0, (char)0xA5); std::atomic<size_t> bump{4096};
    PackDst d{&bump, heap.data(), heap.size(), -1};
    const int rc = pack_window(&wf.w, o, out, h, err, grid, first.empty() ? nullptr : &cache, use_dst ? &d : nullptr, all_blocks);
    if (rc != UVS_OK) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
    const char* blob = d.off >= 0 ? heap.data() + d.off : out.data();
    DevWin b; std::memcpy(&b, blob, sizeof(b));
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(blob, 1, (size_t)h.blob_bytes, f) != (size_t)h.blob_bytes || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::printf("ok %d %d %d %d %d %d %d %d %d %d %d %d %lld %d %d %d\n", h.blob_bytes, h.ws_doubles, h.n_chunks, h.n_pt_obs, h.n_relo, h.pt_rec, h.pt_xslots, h.max_chunk_doubles,
                (int)UVS_S_DOUBLES, h.n_parts, h.n_cimg, h.n_pblk, (long long)b.out_host, b.cur_sel, hit ? 1 : 0, d.off >= 0 ? 1 : 0);
    return 0;
}
