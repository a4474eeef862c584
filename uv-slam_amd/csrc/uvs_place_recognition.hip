// uvs_place_recognition.hip -- place recognition of loop closure (reference pose_graph/src/pose_graph.cpp:304-386 detectLoop;
// ThirdParty/DBoW/TemplatedVocabulary.h:1065-1121, 1217-1258 transform; TemplatedDatabase.h:656-723 queryL1; BowVector.cpp:34-84 addWeight,
// normalize) behind the uvs_pr_* calls of include/uvs_solver.h.  gfx950, one stream per handle.  Integer arithmetic, and FP64 adds, subtracts
// and divides in the reference's order; this unit is compiled with -ffp-contract=off, so they round as written, which is what tests/pr_ref.py
// (the numpy restatement, the pin) does.
//
// The vocabulary is renumbered on the host into SLOTS, breadth first with the children of a node in the order of their records, so that the
// children of a node are consecutive slots: child_off[slot] is the first, child_cnt[slot] their number (0: a leaf), and the descriptors of the
// up to 16 children a descent step compares are 512 consecutive bytes.  Kernels:
//   k_pr_descend   A GROUP OF 16 LANES PER DESCRIPTOR, a lane per child: four 64-bit popcounts, the key (distance << 8 | child rank), its
//                  minimum over the group by four xor-shuffles (a tie goes to the lower rank = the earlier child).  Every level is read
//                  through L2: the top levels of the tree are touched by every descriptor of the call and stay cached.
//   k_pr_bow       a workgroup per keyframe: the word ids (stop words replaced by a sentinel) sorted in LDS (bitonic), the heads of the runs
//                  compacted in order (a scan), a thread per distinct word does v = w, v += w .. once per occurrence, wave 0 sums |v| in
//                  ascending word id (64 values per load, one add after the other), every value is divided by the norm.
//   k_pr_score     a workgroup per 4 .. 64 database entries and query, the query vector in LDS; A WAVE PER ENTRY: 64 consecutive words of the
//                  entry per step, each searched in the query (binary search in LDS), the wave's ballot names the common words and the
//                  terms are added in lane order = ascending word id.  Writes s(e) and the number of common words of every entry.
// The eligible entries' scores are downloaded; the host orders the hits by (s, id) and cuts the list.  No kernel uses scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_handle.h"

namespace uvspr {

constexpr int kThreads = 256;                     // every kernel: 4 waves
constexpr int kGroup = UVS_PR_MAX_K;              // lanes of a descriptor's group in k_pr_descend
constexpr int kMaxF = UVS_LC_MAX_OLD;             // most descriptors of a keyframe
constexpr int kMaxEntriesPerBlock = 64;           // k_pr_score: at most 16 entries per wave, see entries_per_block()
constexpr uint32_t kStop = 0x7FFFFFFFu;           // sort key of a stop word and of the padding
static_assert(kGroup == 16 && kThreads % kGroup == 0, "a 16-lane group per descriptor");
static_assert(kMaxF == 4096 && kMaxF % kThreads == 0, "k_pr_bow sorts up to 4096 keys in LDS");

struct PrFrame { int off, n, max_id, pad; };      // first descriptor in the packed arrays, count, the query's max_id

// ---- transform, step 1: descriptor -> leaf
__global__ void __launch_bounds__(kThreads) k_pr_descend(const unsigned long long* __restrict__ desc, int total, int L,
                                                       const unsigned long long* __restrict__ node_desc, const int* __restrict__ child_off,
                                                       const int* __restrict__ child_cnt, const int* __restrict__ node_word,
                                                       const double* __restrict__ node_weight, int* __restrict__ words, double* __restrict__ weights) {
    const int item = blockIdx.x * (kThreads / kGroup) + (threadIdx.x / kGroup), r = threadIdx.x % kGroup;
    const bool live = item < total;                           // uniform over the group
    unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (live) { const unsigned long long* p = desc + 4 * (size_t)item; d0 = p[0]; d1 = p[1]; d2 = p[2]; d3 = p[3]; }
    int node = 0;
    for (int level = 0; level < L; ++level) {                 // every lane of the wave runs every level: the shuffles below are never divergent
        const int cnt = live ? child_cnt[node] : 0, off = live ? child_off[node] : 0;
        if (!__any(cnt > 0)) break;                           // wave-uniform
        unsigned key = 0xFFFFFFFFu;
        if (r < cnt) {
            const unsigned long long* c = node_desc + 4 * (size_t)(off + r);
            const int dist = __popcll(c[0] ^ d0) + __popcll(c[1] ^ d1) + __popcll(c[2] ^ d2) + __popcll(c[3] ^ d3);
            key = ((unsigned)dist << 8) | (unsigned)r;
        }
#pragma unroll
        for (int m = kGroup / 2; m > 0; m >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, m, kGroup));
        if (cnt > 0) node = off + (int)(key & 255u);
    }
    if (live && r == 0) { words[item] = node_word[node]; weights[item] = node_weight[node]; }
}

// ---- transform, step 2: the keyframe's bag-of-words vector
__global__ void __launch_bounds__(kThreads) k_pr_bow(const PrFrame* __restrict__ frames, const int* __restrict__ words, const double* __restrict__ weights,
                                                   const double* __restrict__ word_weight, int max_features, int* __restrict__ bow_n,
                                                   int* __restrict__ bow_words, double* __restrict__ bow_values) {
    __shared__ uint32_t sKey[kMaxF];
    __shared__ double sVal[kMaxF];
    __shared__ uint16_t sPos[kMaxF + 2];
    __shared__ int sPart[kThreads];
    __shared__ double sNorm;
    const PrFrame F = frames[blockIdx.x];
    const int tid = threadIdx.x, n = F.n;                     // n <= max_features <= kMaxF (checked by the host)
    if (n == 0) { if (tid == 0) bow_n[blockIdx.x] = 0; return; }
    int N = 2;
    while (N < n) N <<= 1;                                    // <= kMaxF
    for (int i = tid; i < N; i += kThreads) sKey[i] = i < n && weights[F.off + i] > 0.0 ? (uint32_t)words[F.off + i] : kStop;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += kThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const uint32_t a = sKey[i], b = sKey[x];
                    if ((a > b) == ((i & k) == 0)) { sKey[i] = b; sKey[x] = a; }
                }
            }
            __syncthreads();
        }
    // heads of the runs (the first stop key is a head too: its position ends the last word's run), compacted in order
    const int chunk = (N + kThreads - 1) / kThreads;
    const int b = min(tid * chunk, N), e = min(b + chunk, N);
    int heads = 0;
    for (int i = b; i < e; ++i) heads += i == 0 || sKey[i] != sKey[i - 1];
    sPart[tid] = heads;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int v = tid >= off ? sPart[tid - off] : 0;
        __syncthreads();
        sPart[tid] += v;
        __syncthreads();
    }
    int run = sPart[tid] - heads;
    for (int i = b; i < e; ++i) if (i == 0 || sKey[i] != sKey[i - 1]) sPos[run++] = (uint16_t)i;
    const int H = sPart[kThreads - 1];
    if (tid == 0) sPos[H] = (uint16_t)N;
    const int U = H - (sKey[N - 1] == kStop ? 1 : 0);         // distinct words of positive weight
    __syncthreads();
    int* out_w = bow_words + (size_t)blockIdx.x * max_features;
    double* out_v = bow_values + (size_t)blockIdx.x * max_features;
    for (int j = tid; j < U; j += kThreads) {
        const int p = sPos[j], len = sPos[j + 1] - p;
        const int word = (int)sKey[p];
        const double w = word_weight[word];
        double v = w;
        for (int c = 1; c < len; ++c) v += w;                 // BowVector::addWeight, once per occurrence
        sVal[j] = v;
        out_w[j] = word;
    }
    __syncthreads();
    if (tid < 64) {                                           // BowVector::normalize: the sum of |v| in ascending word id
        double s = 0.0;
        for (int base = 0; base < U; base += 64) {
            const double x = base + tid < U ? fabs(sVal[base + tid]) : 0.0;      // + 0.0 past the end changes nothing: s >= 0
#pragma unroll 8
            for (int j = 0; j < 64; ++j) s += __shfl(x, j);
        }
        if (tid == 0) { sNorm = s; bow_n[blockIdx.x] = U; }
    }
    __syncthreads();
    const double norm = sNorm;
    for (int j = tid; j < U; j += kThreads) out_v[j] = norm > 0.0 ? sVal[j] / norm : sVal[j];
}

// ---- query: s(e) and the number of common words of every entry, for every query of the call
__global__ void __launch_bounds__(kThreads) k_pr_score(const PrFrame* __restrict__ frames, const int* __restrict__ bow_n, const int* __restrict__ bow_words,
                                                     const double* __restrict__ bow_values, int max_features, int n_entries, int per_block,
                                                     const long long* __restrict__ db_off, const int* __restrict__ db_words,
                                                     const double* __restrict__ db_values, double* __restrict__ out_s, int* __restrict__ out_cnt) {
    __shared__ int sQw[kMaxF];
    __shared__ double sQv[kMaxF];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = bow_n[q], max_id = frames[q].max_id;
    for (int i = tid; i < nq; i += kThreads) { sQw[i] = bow_words[(size_t)q * max_features + i]; sQv[i] = bow_values[(size_t)q * max_features + i]; }
    __syncthreads();
    const int e_end = min((int)(blockIdx.x + 1) * per_block, n_entries);
    for (int e = blockIdx.x * per_block + wave; e < e_end; e += kThreads / 64) {      // wave-uniform
        const bool eligible = e < max_id || max_id == -1 || e == n_entries - 1;
        double s = 0.0;
        int hits = 0;
        if (eligible && nq > 0) {
            const long long b = db_off[e];
            const int len = (int)(db_off[e + 1] - b);
            for (int c = 0; c < len; c += 64) {
                const int i = c + lane;
                double term = 0.0;
                bool hit = false;
                if (i < len) {
                    const int w = db_words[b + i];
                    int lo = 0, hi = nq;                      // the first query word >= w
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sQw[mid] < w) lo = mid + 1; else hi = mid; }
                    if (lo < nq && sQw[lo] == w) {
                        const double qv = sQv[lo], dv = db_values[b + i];
                        term = fabs(qv - dv) - fabs(qv) - fabs(dv);
                        hit = true;
                    }
                }
                unsigned long long m = __ballot(hit);
                while (m) {                                   // the common words of this step, in ascending word id
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const double t = __shfl(term, j);
                    s = hits ? s + t : t;
                    ++hits;
                }
            }
        }
        if (lane == 0) { out_s[(size_t)q * n_entries + e] = s; out_cnt[(size_t)q * n_entries + e] = hits; }
    }
}

}  // namespace uvspr

using namespace uvspr;

struct uvs_place_recognizer : UvsHandle {
    int L = 0, n_slots = 0, n_words = 0, max_features = 0;
    float ms_total = 0.f, ms_transform = 0.f, ms_query = 0.f;      // uvs_pr_last_device_ms
    hipEvent_t ev_mid = nullptr, ev_q = nullptr;                   // after the transform / after the query's download
    // the vocabulary by slot
    DevBuf<uint64_t> d_node_desc;
    DevBuf<int> d_child_off, d_child_cnt, d_node_word;
    DevBuf<double> d_node_weight, d_word_weight;
    // one call's transform: frames | descriptors in, words / weights per descriptor, the vectors (strided by max_features)
    DevBuf<char> d_in;
    PinnedBuf<char> h_in;
    DevBuf<int> d_words, d_bow_n, d_bow_words;
    DevBuf<double> d_weights, d_bow_values;
    PinnedBuf<char> h_out;                                         // bow_n | words | weights | bow_words | bow_values
    // one call's query: s and the common-word count of every (query, entry)
    DevBuf<double> d_score;
    DevBuf<int> d_cnt;
    PinnedBuf<char> h_score;
    // the database: entry-major, append-only
    std::vector<long long> h_off{0};                               // h_off[e] .. h_off[e + 1]: the words of entry e
    size_t cap_entries = 0, cap_items = 0;
    DevBuf<long long> d_off;
    DevBuf<int> d_db_words;
    DevBuf<double> d_db_values;
    ~uvs_place_recognizer() {
        if (ev_mid) (void)hipEventDestroy(ev_mid);
        if (ev_q) (void)hipEventDestroy(ev_q);
    }
    int size() const { return (int)h_off.size() - 1; }
};

namespace {

struct VocCheck {                      // what the check works out and uvs_pr_create uploads
    std::vector<int> slot_of;          // node id -> slot
    std::vector<int> child_off, child_cnt, node_word;
    std::vector<double> node_weight, word_weight;
    std::vector<uint64_t> node_desc;
};

int voc_fail(std::string& msg, const std::string& what) { msg = "vocabulary: " + what; return UVS_ERR_INVALID_ARG; }

int check_vocabulary(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* node_id, const int32_t* parent_id, const double* weight,
                     const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id, std::string& msg, VocCheck* out) {
    msg.clear();
    if (scoring != 0 || weighting != 0) { msg = "vocabulary: only weightingType 0 (TF_IDF) with scoringType 0 (L1_NORM) is built"; return UVS_ERR_UNSUPPORTED; }
    if (k < 1 || k > UVS_PR_MAX_K) return voc_fail(msg, "k outside 1 .. UVS_PR_MAX_K");
    if (L < 1 || L > UVS_PR_MAX_L) return voc_fail(msg, "L outside 1 .. UVS_PR_MAX_L");
    if (n_nodes < 1) return voc_fail(msg, "the root has no children");
    if (n_words < 1) return voc_fail(msg, "no words");
    if (!node_id || !parent_id || !weight || !descriptor || !word_node_id || !word_id) return voc_fail(msg, "null array");
    const size_t S = (size_t)n_nodes + 1;
    std::vector<int> rec(S, -1);                               // node id -> record
    for (int i = 0; i < n_nodes; ++i) {
        const int id = node_id[i];
        if (id < 1 || id > n_nodes) return voc_fail(msg, "record " + std::to_string(i) + ": node id outside 1 .. n_nodes");
        if (rec[id] >= 0) return voc_fail(msg, "node id " + std::to_string(id) + " given twice");
        rec[id] = i;
    }
    std::vector<int> cnt(S, 0);
    for (int i = 0; i < n_nodes; ++i) {
        const int p = parent_id[i];
        if (p < 0 || p > n_nodes) return voc_fail(msg, "node " + std::to_string(node_id[i]) + ": its parent does not exist");
        if (!std::isfinite(weight[i]) || weight[i] < 0.0) return voc_fail(msg, "node " + std::to_string(node_id[i]) + ": a weight that is negative or not finite");
        ++cnt[p];
    }
    if (cnt[0] == 0) return voc_fail(msg, "the root has no children");
    for (size_t id = 0; id < S; ++id)
        if (cnt[id] > UVS_PR_MAX_K) return voc_fail(msg, "node " + std::to_string(id) + " has more than UVS_PR_MAX_K children");
    // depth of every node; a walk towards the root that meets a node of the same walk is a cycle
    std::vector<int> depth(S, -1), mark(S, -1);
    depth[0] = 0;
    std::vector<int> path;
    for (int id = 1; id <= n_nodes; ++id) {
        path.clear();
        int v = id;
        while (depth[v] < 0) {
            if (mark[v] == id) return voc_fail(msg, "node " + std::to_string(v) + " is on a cycle");
            mark[v] = id; path.push_back(v);
            v = parent_id[rec[v]];
        }
        int d = depth[v];
        for (size_t i = path.size(); i-- > 0;) depth[path[i]] = ++d;
        if (depth[id] > L) return voc_fail(msg, "node " + std::to_string(id) + " is deeper than L");
    }
    // words
    std::vector<int> word_of(S, -1), node_of_word((size_t)n_words, -1);
    for (int i = 0; i < n_words; ++i) {
        const int nid = word_node_id[i], wid = word_id[i];
        if (nid < 1 || nid > n_nodes) return voc_fail(msg, "word record " + std::to_string(i) + ": node id outside 1 .. n_nodes");
        if (wid < 0 || wid >= n_words) return voc_fail(msg, "word record " + std::to_string(i) + ": word id outside 0 .. n_words - 1");
        if (node_of_word[wid] >= 0) return voc_fail(msg, "word id " + std::to_string(wid) + " given twice");
        if (word_of[nid] >= 0) return voc_fail(msg, "node " + std::to_string(nid) + " has two words");
        if (cnt[nid] > 0) return voc_fail(msg, "word " + std::to_string(wid) + " is on an inner node");
        node_of_word[wid] = nid; word_of[nid] = wid;
    }
    for (int id = 1; id <= n_nodes; ++id)
        if (cnt[id] == 0 && word_of[id] < 0) return voc_fail(msg, "leaf " + std::to_string(id) + " has no word");
    if (!out) return UVS_OK;
    // slots: breadth first, the children of a node in the order of their records
    std::vector<int> child_start(S + 1, 0);
    for (size_t id = 0; id < S; ++id) child_start[id + 1] = child_start[id] + cnt[id];
    std::vector<int> fill(child_start.begin(), child_start.end() - 1), children((size_t)n_nodes);
    for (int i = 0; i < n_nodes; ++i) children[fill[parent_id[i]]++] = node_id[i];
    std::vector<int> order;                                    // slot -> node id
    order.reserve(S);
    order.push_back(0);
    out->slot_of.assign(S, -1);
    out->slot_of[0] = 0;
    out->child_off.assign(S, 0); out->child_cnt.assign(S, 0);
    for (size_t s = 0; s < order.size(); ++s) {
        const int id = order[s];
        out->child_off[s] = (int)order.size(); out->child_cnt[s] = cnt[id];
        for (int c = 0; c < cnt[id]; ++c) { const int ch = children[child_start[id] + c]; out->slot_of[ch] = (int)order.size(); order.push_back(ch); }
    }
    out->node_word.assign(S, -1); out->node_weight.assign(S, 0.0); out->node_desc.assign(4 * S, 0);
    out->word_weight.assign((size_t)n_words, 0.0);
    for (size_t s = 1; s < S; ++s) {                           // every node is reached: no cycle, every parent exists
        const int id = order[s], i = rec[id];
        out->node_word[s] = word_of[id]; out->node_weight[s] = weight[i];
        for (int c = 0; c < 4; ++c) out->node_desc[4 * s + c] = descriptor[4 * (size_t)i + c];
        if (word_of[id] >= 0) out->word_weight[word_of[id]] = weight[i];
    }
    return UVS_OK;
}

template <class T>
int upload(uvs_place_recognizer* h, DevBuf<T>& d, const std::vector<T>& v) {
    int rc = d.ensure(std::max<size_t>(v.size() * sizeof(T), 16), h->err);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return UVS_OK;
}

// a device buffer of the database grows to `bytes`, keeping its first `used` bytes: a new buffer, a device-to-device copy, the old one freed
template <class T>
int grow_keep(uvs_place_recognizer* h, DevBuf<T>& d, size_t bytes, size_t used) {
    DevBuf<T> fresh;
    const int rc = fresh.ensure(bytes, h->err);
    if (rc != UVS_OK) return rc;
    if (used) UVS_HIP(h->err, hipMemcpyAsync(fresh, d, used, hipMemcpyDeviceToDevice, h->st));
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    d = std::move(fresh);                                      // swaps; `fresh` frees the old buffer
    return UVS_OK;
}

int db_reserve(uvs_place_recognizer* h, size_t entries, size_t items) {
    if (entries > h->cap_entries) {
        size_t cap = h->cap_entries;
        while (cap < entries) cap *= 2;
        const int rc = grow_keep(h, h->d_off, (cap + 1) * sizeof(long long), h->h_off.size() * sizeof(long long));
        if (rc != UVS_OK) return rc;
        h->cap_entries = cap;
    }
    if (items > h->cap_items) {
        size_t cap = h->cap_items;
        while (cap < items) cap *= 2;
        const size_t used = (size_t)h->h_off.back();
        int rc = grow_keep(h, h->d_db_words, cap * sizeof(int), used * sizeof(int));
        if (rc == UVS_OK) rc = grow_keep(h, h->d_db_values, cap * sizeof(double), used * sizeof(double));
        if (rc != UVS_OK) return rc;
        h->cap_items = cap;
    }
    return UVS_OK;
}

struct OutLayout { size_t words, weights, bow_words, bow_values, total; };
inline OutLayout out_layout(size_t n_frames, size_t total, size_t max_features) {
    OutLayout L;
    L.words = align_up(n_frames * 4, 256);
    L.weights = align_up(L.words + total * 4, 256);
    L.bow_words = align_up(L.weights + total * 8, 256);
    L.bow_values = align_up(L.bow_words + n_frames * max_features * 4, 256);
    L.total = L.bow_values + n_frames * max_features * 8;
    return L;
}

int check_frames(uvs_place_recognizer* h, const std::string& fn, int n_frames, const int32_t* n_features, const uint64_t* descriptors, size_t& total) {
    h->err.clear();
    if (n_frames < 1 || !n_features) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_frames > UVS_PR_MAX_FRAMES) { h->err = fn + ": more than UVS_PR_MAX_FRAMES keyframes"; return UVS_ERR_CAPACITY; }
    total = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (n_features[f] < 0) { h->err = fn + ": a negative count"; return UVS_ERR_INVALID_ARG; }
        if (n_features[f] > h->max_features) { h->err = fn + ": more descriptors than max_features"; return UVS_ERR_CAPACITY; }
        total += (size_t)n_features[f];
    }
    if (total && !descriptors) { h->err = fn + ": null descriptors"; return UVS_ERR_INVALID_ARG; }
    return UVS_OK;
}

// upload and the two transform kernels on the handle's stream, between ev0 and ev_mid; no synchronization
int enqueue_transform(uvs_place_recognizer* h, int n_frames, const int32_t* n_features, const uint64_t* descriptors, const int32_t* max_id, size_t total) {
    const size_t o_desc = align_up(UVS_PR_MAX_FRAMES * sizeof(PrFrame), 256);
    PrFrame* hf = reinterpret_cast<PrFrame*>(h->h_in.get());
    int off = 0;
    for (int f = 0; f < n_frames; ++f) { hf[f] = PrFrame{off, n_features[f], max_id ? max_id[f] : -1, 0}; off += n_features[f]; }
    if (total) std::memcpy(h->h_in + o_desc, descriptors, total * 32);
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, o_desc + total * 32, hipMemcpyHostToDevice, st));
    const PrFrame* dF = reinterpret_cast<const PrFrame*>(h->d_in.get());
    const unsigned long long* dDesc = reinterpret_cast<const unsigned long long*>(h->d_in + o_desc);
    if (total) {
        const int per_block = kThreads / kGroup;
        k_pr_descend<<<(unsigned)((total + per_block - 1) / per_block), kThreads, 0, st>>>(dDesc, (int)total, h->L, reinterpret_cast<const unsigned long long*>(h->d_node_desc.get()), h->d_child_off, h->d_child_cnt,
                                                                                          h->d_node_word, h->d_node_weight, h->d_words, h->d_weights);
    }
    k_pr_bow<<<n_frames, kThreads, 0, st>>>(dF, h->d_words, h->d_weights, h->d_word_weight, h->max_features, h->d_bow_n, h->d_bow_words, h->d_bow_values);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_bow_n, (size_t)n_frames * 4, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev_mid, st));
    return UVS_OK;
}

// Entries of one workgroup of k_pr_score.  A wave walks its entries one after the other and an entry is a chain of dependent loads, so a small
// database is spread over as many workgroups as it has groups of four entries (a wave each); from 8192 entries on a wave takes more, up to 16,
// so that the query vector is not staged into LDS more often than the entries' own words are read.  The result does not depend on it.
inline int entries_per_block(int n) {
    const int want = (n + 2047) / 2048;                        // about 2048 workgroups
    return std::min(kMaxEntriesPerBlock, std::max(4, (want + 3) / 4 * 4));
}

// the score kernel for the call's n_frames queries against the n entries of the database and the download, up to ev_q; no synchronization
int enqueue_score(uvs_place_recognizer* h, int n_frames, int n) {
    const size_t cells = (size_t)n_frames * n;
    int rc = h->d_score.ensure(cells * 8, h->err, grow_half);
    if (rc == UVS_OK) rc = h->d_cnt.ensure(cells * 4, h->err, grow_half);
    if (rc == UVS_OK) rc = h->h_score.ensure(align_up(cells * 8, 256) + cells * 4, h->err, grow_pinned);
    if (rc != UVS_OK) return rc;
    hipStream_t st = h->st;
    const PrFrame* dF = reinterpret_cast<const PrFrame*>(h->d_in.get());
    const int per_block = entries_per_block(n);
    k_pr_score<<<dim3((unsigned)((n + per_block - 1) / per_block), n_frames), kThreads, 0, st>>>(
        dF, h->d_bow_n, h->d_bow_words, h->d_bow_values, h->max_features, n, per_block, h->d_off, h->d_db_words, h->d_db_values, h->d_score, h->d_cnt);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_score, h->d_score, cells * 8, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->h_score + align_up(cells * 8, 256), h->d_cnt, cells * 4, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev_q, st));
    return UVS_OK;
}

// the hits of query f in ascending (s, id), cut to max_results (0: all); Score = -s / 2
int rank_results(const uvs_place_recognizer* h, int n_frames, int f, int n, int max_results, int32_t* ids, double* scores) {
    const size_t cells = (size_t)n_frames * n;
    const double* s = reinterpret_cast<const double*>(h->h_score.get()) + (size_t)f * n;
    const int* cnt = reinterpret_cast<const int*>(h->h_score + align_up(cells * 8, 256)) + (size_t)f * n;
    std::vector<int> hit;
    for (int e = 0; e < n; ++e) if (cnt[e] > 0) hit.push_back(e);
    const size_t keep = max_results > 0 ? std::min(hit.size(), (size_t)max_results) : hit.size();
    std::partial_sort(hit.begin(), hit.begin() + keep, hit.end(), [s](int a, int b) { return s[a] < s[b] || (s[a] == s[b] && a < b); });
    for (size_t i = 0; i < keep; ++i) { ids[i] = hit[i]; scores[i] = -s[hit[i]] / 2.0; }
    return (int)keep;
}

// appends the vectors of the call's frames (bow_n in h_out) to the database, in order
int append_frames(uvs_place_recognizer* h, int n_frames, int32_t* entry_ids) {
    const int* bow_n = reinterpret_cast<const int*>(h->h_out.get());
    long long items = h->h_off.back();
    for (int f = 0; f < n_frames; ++f) items += bow_n[f];
    const int rc = db_reserve(h, (size_t)h->size() + n_frames, (size_t)items);
    if (rc != UVS_OK) return rc;
    const size_t first = h->h_off.size() - 1;
    for (int f = 0; f < n_frames; ++f) {
        const long long at = h->h_off.back();
        if (bow_n[f]) {
            UVS_HIP(h->err, hipMemcpyAsync(h->d_db_words + at, h->d_bow_words + (size_t)f * h->max_features, (size_t)bow_n[f] * 4, hipMemcpyDeviceToDevice, h->st));
            UVS_HIP(h->err, hipMemcpyAsync(h->d_db_values + at, h->d_bow_values + (size_t)f * h->max_features, (size_t)bow_n[f] * 8, hipMemcpyDeviceToDevice, h->st));
        }
        if (entry_ids) entry_ids[f] = h->size();
        h->h_off.push_back(at + bow_n[f]);
    }
    UVS_HIP(h->err, hipMemcpyAsync(h->d_off + first, h->h_off.data() + first, (h->h_off.size() - first) * sizeof(long long), hipMemcpyHostToDevice, h->st));
    return UVS_OK;
}

int finish(uvs_place_recognizer* h, bool queried) {
    UVS_HIP(h->err, hipEventRecord(h->ev1, h->st));
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->ms_total, h->ev0, h->ev1));
    UVS_HIP(h->err, hipEventElapsedTime(&h->ms_transform, h->ev0, h->ev_mid));
    h->ms_query = 0.f;
    if (queried) UVS_HIP(h->err, hipEventElapsedTime(&h->ms_query, h->ev_mid, h->ev_q));
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_pr_check_vocabulary(int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t* node_id, const int32_t* parent_id,
                            const double* weight, const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id,
                            char* message, int message_capacity) {
    std::string msg;
    const int rc = check_vocabulary(k, L, scoring_type, weighting_type, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_node_id, word_id, msg, nullptr);
    if (message && message_capacity > 0) std::snprintf(message, (size_t)message_capacity, "%s", msg.c_str());
    return rc;
}

int uvs_pr_create(int device, int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t* node_id, const int32_t* parent_id,
                  const double* weight, const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id,
                  int max_features, int initial_entries, uvs_place_recognizer** out) {
    if (!out) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_features < 1 || initial_entries < 1) return UVS_ERR_INVALID_ARG;
    if (max_features > UVS_LC_MAX_OLD) return UVS_ERR_CAPACITY;
    VocCheck V;
    std::string msg;
    int rc = check_vocabulary(k, L, scoring_type, weighting_type, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_node_id, word_id, msg, &V);
    if (rc != UVS_OK) { if (!msg.empty()) std::fprintf(stderr, "uvs_pr_create: %s\n", msg.c_str()); return rc; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_place_recognizer* h = new uvs_place_recognizer();
    h->L = L; h->n_slots = n_nodes + 1; h->n_words = n_words; h->max_features = max_features;
    const size_t B = UVS_PR_MAX_FRAMES, T = B * (size_t)max_features;
    const size_t in_bytes = align_up(B * sizeof(PrFrame), 256) + T * 32;
    h->cap_entries = (size_t)initial_entries;
    h->cap_items = (size_t)initial_entries * 256;              // doubled as the entries' words come in
    rc = h->open(device);
    if (rc == UVS_OK && (hipEventCreate(&h->ev_mid) != hipSuccess || hipEventCreate(&h->ev_q) != hipSuccess)) rc = UVS_ERR_HIP;
    if (rc == UVS_OK && (rc = upload(h, h->d_node_desc, V.node_desc)) == UVS_OK && (rc = upload(h, h->d_child_off, V.child_off)) == UVS_OK &&
        (rc = upload(h, h->d_child_cnt, V.child_cnt)) == UVS_OK && (rc = upload(h, h->d_node_word, V.node_word)) == UVS_OK &&
        (rc = upload(h, h->d_node_weight, V.node_weight)) == UVS_OK && (rc = upload(h, h->d_word_weight, V.word_weight)) == UVS_OK &&
        (rc = h->d_in.ensure(in_bytes, h->err)) == UVS_OK && (rc = h->h_in.ensure(in_bytes, h->err)) == UVS_OK &&
        (rc = h->d_words.ensure(T * 4, h->err)) == UVS_OK && (rc = h->d_weights.ensure(T * 8, h->err)) == UVS_OK &&
        (rc = h->d_bow_n.ensure(B * 4, h->err)) == UVS_OK && (rc = h->d_bow_words.ensure(T * 4, h->err)) == UVS_OK &&
        (rc = h->d_bow_values.ensure(T * 8, h->err)) == UVS_OK && (rc = h->h_out.ensure(out_layout(B, T, max_features).total, h->err)) == UVS_OK &&
        (rc = h->d_off.ensure((h->cap_entries + 1) * sizeof(long long), h->err)) == UVS_OK &&
        (rc = h->d_db_words.ensure(h->cap_items * 4, h->err)) == UVS_OK && (rc = h->d_db_values.ensure(h->cap_items * 8, h->err)) == UVS_OK) {
        const long long zero = 0;
        const hipError_t e = hipMemcpy(h->d_off, &zero, sizeof zero, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(h->err, e, "hipMemcpy");
    }
    if (rc != UVS_OK) { uvs_pr_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_pr_destroy(uvs_place_recognizer* h) { if (h) { h->close(); delete h; } }

const char* uvs_pr_last_error(const uvs_place_recognizer* h) { return h ? h->err.c_str() : "null place recognizer"; }

int uvs_pr_size(const uvs_place_recognizer* h) { return h ? h->size() : 0; }

int uvs_pr_clear(uvs_place_recognizer* h) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    h->h_off.assign(1, 0);                                     // d_off[0] is 0 since uvs_pr_create
    return UVS_OK;
}

double uvs_pr_last_device_ms(const uvs_place_recognizer* h, int part) {
    if (!h) return 0.0;
    return part == 0 ? (double)h->ms_total : part == 1 ? (double)h->ms_transform : part == 2 ? (double)h->ms_query : 0.0;
}

int uvs_pr_transform(uvs_place_recognizer* h, int n_frames, const int32_t* n_features, const uint64_t* descriptors, int32_t* words_out,
                     double* weights_out, int32_t* bow_n, int32_t* bow_words, double* bow_values) {
    if (!h) return UVS_ERR_INVALID_ARG;
    size_t total = 0;
    int rc = check_frames(h, "uvs_pr_transform", n_frames, n_features, descriptors, total);
    if (rc != UVS_OK) return rc;
    if (!words_out || !weights_out || !bow_n || !bow_words || !bow_values) { h->err = "uvs_pr_transform: null pointer"; return UVS_ERR_INVALID_ARG; }
    if ((rc = enqueue_transform(h, n_frames, n_features, descriptors, nullptr, total)) != UVS_OK) return rc;
    const OutLayout O = out_layout(n_frames, total, h->max_features);
    const size_t strided = (size_t)n_frames * h->max_features;
    if (total) {
        UVS_HIP(h->err, hipMemcpyAsync(h->h_out + O.words, h->d_words, total * 4, hipMemcpyDeviceToHost, h->st));
        UVS_HIP(h->err, hipMemcpyAsync(h->h_out + O.weights, h->d_weights, total * 8, hipMemcpyDeviceToHost, h->st));
        UVS_HIP(h->err, hipMemcpyAsync(h->h_out + O.bow_words, h->d_bow_words, strided * 4, hipMemcpyDeviceToHost, h->st));
        UVS_HIP(h->err, hipMemcpyAsync(h->h_out + O.bow_values, h->d_bow_values, strided * 8, hipMemcpyDeviceToHost, h->st));
    }
    if ((rc = finish(h, false)) != UVS_OK) return rc;
    std::memcpy(bow_n, h->h_out, (size_t)n_frames * 4);
    if (total) {
        std::memcpy(words_out, h->h_out + O.words, total * 4);
        std::memcpy(weights_out, h->h_out + O.weights, total * 8);
    }
    for (int f = 0; f < n_frames; ++f) {                       // the strided vectors: the written entries only
        const size_t o = (size_t)f * h->max_features, n = (size_t)bow_n[f];
        if (!n) continue;
        std::memcpy(bow_words + o, h->h_out + O.bow_words + o * 4, n * 4);
        std::memcpy(bow_values + o, h->h_out + O.bow_values + o * 8, n * 8);
    }
    return UVS_OK;
}

int uvs_pr_add(uvs_place_recognizer* h, int n_frames, const int32_t* n_features, const uint64_t* descriptors, int32_t* entry_ids) {
    if (!h) return UVS_ERR_INVALID_ARG;
    size_t total = 0;
    int rc = check_frames(h, "uvs_pr_add", n_frames, n_features, descriptors, total);
    if (rc != UVS_OK) return rc;
    if (!entry_ids) { h->err = "uvs_pr_add: null pointer"; return UVS_ERR_INVALID_ARG; }
    if ((rc = enqueue_transform(h, n_frames, n_features, descriptors, nullptr, total)) != UVS_OK) return rc;
    UVS_HIP(h->err, hipStreamSynchronize(h->st));              // bow_n: the sizes of the new entries
    if ((rc = append_frames(h, n_frames, entry_ids)) != UVS_OK) return rc;
    return finish(h, false);
}

int uvs_pr_query(uvs_place_recognizer* h, int n_frames, const int32_t* n_features, const uint64_t* descriptors, int max_results,
                 const int32_t* max_id, int32_t* n_results, int32_t* ids, double* scores) {
    if (!h) return UVS_ERR_INVALID_ARG;
    size_t total = 0;
    int rc = check_frames(h, "uvs_pr_query", n_frames, n_features, descriptors, total);
    if (rc != UVS_OK) return rc;
    if (max_results < 0 || !max_id || !n_results || !ids || !scores) { h->err = "uvs_pr_query: null pointer or a negative max_results"; return UVS_ERR_INVALID_ARG; }
    const int n = h->size();
    if ((rc = enqueue_transform(h, n_frames, n_features, descriptors, max_id, total)) != UVS_OK) return rc;
    if (n > 0 && (rc = enqueue_score(h, n_frames, n)) != UVS_OK) return rc;
    if ((rc = finish(h, n > 0)) != UVS_OK) return rc;
    const size_t stride = max_results > 0 ? (size_t)max_results : (size_t)n;
    for (int f = 0; f < n_frames; ++f) n_results[f] = n > 0 ? rank_results(h, n_frames, f, n, max_results, ids + f * stride, scores + f * stride) : 0;
    return UVS_OK;
}

int uvs_pr_detect(uvs_place_recognizer* h, int n_features, const uint64_t* descriptors, int frame_index, int32_t* loop_index, int32_t* n_results,
                  int32_t* ids, double* scores) {
    if (!h) return UVS_ERR_INVALID_ARG;
    size_t total = 0;
    int rc = check_frames(h, "uvs_pr_detect", 1, &n_features, descriptors, total);
    if (rc != UVS_OK) return rc;
    if (!loop_index || !n_results || !ids || !scores) { h->err = "uvs_pr_detect: null pointer"; return UVS_ERR_INVALID_ARG; }
    const int n = h->size();
    const int32_t max_id = frame_index - 50;                   // pose_graph.cpp:327
    if ((rc = enqueue_transform(h, 1, &n_features, descriptors, &max_id, total)) != UVS_OK) return rc;
    if (n > 0 && (rc = enqueue_score(h, 1, n)) != UVS_OK) return rc;
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    if ((rc = append_frames(h, 1, nullptr)) != UVS_OK) return rc;      // :330 db.add
    if ((rc = finish(h, n > 0)) != UVS_OK) return rc;
    const int m = n > 0 ? rank_results(h, 1, 0, n, UVS_PR_DETECT_RESULTS, ids, scores) : 0;
    *n_results = m;
    bool find_loop = false;                                    // :352-386
    if (m >= 1 && scores[0] > 0.05)
        for (int i = 1; i < m; ++i) if (scores[i] > 0.015) find_loop = true;
    int min_index = -1;
    if (find_loop && frame_index > 50)
        for (int i = 0; i < m; ++i)
            if (min_index == -1 || (ids[i] < min_index && scores[i] > 0.015)) min_index = ids[i];
    *loop_index = min_index;
    return UVS_OK;
}

}  // extern "C"
