// line_ahead_rule.cpp -- the placement rule of csrc/uvs_layout.h (uvs_line_ahead_base: where a line chunk's records go when its pass A runs under the previous
// chunk's gather walk) as a stand-alone host program.  No HIP; the program of tests/test_line_ahead_rule.py and of sanitizer runs of the rule:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/line_ahead_rule.cpp -o line_ahead_rule
//   line_ahead_rule chunks <blob of tools/pack_dump>   -> "<pt_rec> <pt_xslots> <n_chunks> <UVS_S_DOUBLES>", then per chunk "<type> <nob> <nlm> <nlist>"
//   line_ahead_rule bases <blob>                       -> per consecutive pair of chunks "<record base of the second, or -1>", chained as linearize_roles chains it
//   line_ahead_rule rule <cur_end> <cur_rec_base> <cur_rec_size> <next_type> <next_nob> <next_nlm> <next_nlist>   -> the base, or -1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../uv-slam_amd/csrc/uvs_layout.h"

struct Chunk { int type, nob, nlm, nlist; };

static bool load(const char* path, DevWin& h, std::vector<Chunk>& chunks) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::vector<char> raw;
    char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) raw.insert(raw.end(), buf, buf + n);
    std::fclose(f);
    if (raw.size() < sizeof(DevWin)) return false;
    std::memcpy(&h, raw.data(), sizeof(h));
    if (h.n_chunks < 0 || h.i_chunks < 0 || ((size_t)h.i_chunks + (size_t)UVS_CHUNK_INTS * h.n_chunks) * 4 > raw.size()) return false;
    for (int q = 0; q < h.n_chunks; ++q) {
        int32_t w[UVS_CHUNK_INTS];
        std::memcpy(w, raw.data() + 4 * ((size_t)h.i_chunks + (size_t)UVS_CHUNK_INTS * q), sizeof(w));
        chunks.push_back({w[0], w[7], w[2] - w[1], w[4]});
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc == 9 && !std::strcmp(argv[1], "rule")) {
        int v[7];
        for (int k = 0; k < 7; ++k) v[k] = std::atoi(argv[2 + k]);
        std::printf("%d\n", uvs_line_ahead_base(v[0], v[1], v[2], v[3], v[4], v[5], v[6]));
        return 0;
    }
    DevWin h; std::vector<Chunk> ch;
    if (argc != 3 || (std::strcmp(argv[1], "chunks") && std::strcmp(argv[1], "bases")) || !load(argv[2], h, ch)) {
        std::fprintf(stderr, "usage: line_ahead_rule chunks|bases <blob>  |  line_ahead_rule rule <7 integers>\n");
        return 2;
    }
    if (!std::strcmp(argv[1], "chunks")) {
        std::printf("%d %d %d %d\n", h.pt_rec, h.pt_xslots, h.n_chunks, (int)UVS_S_DOUBLES);
        for (const Chunk& c : ch) std::printf("%d %d %d %d\n", c.type, c.nob, c.nlm, c.nlist);
        return 0;
    }
    int rb = 0;      // record base of the current chunk (the first chunk of a linearization never runs ahead)
    for (size_t q = 0; q + 1 < ch.size(); ++q) {
        const Chunk& c = ch[q]; const Chunk& n = ch[q + 1];
        const int nb = uvs_line_ahead_base(uvs_chunk_end(c.type, c.nob, c.nlm, c.nlist, h.pt_rec, h.pt_xslots), rb, c.nob * (c.type == 0 ? h.pt_rec : UVS_LN_REC), n.type, n.nob, n.nlm, n.nlist);
        std::printf("%d\n", nb);
        rb = nb > 0 ? nb : 0;
    }
    return 0;
}
