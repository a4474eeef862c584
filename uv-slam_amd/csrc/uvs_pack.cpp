// uvs_pack.cpp -- host packing: uvs_window -> blob (interface and build notes: uvs_pack.h).  No HIP in this file.
//
// pack_window runs named stages over one PackPlan:
//   validate_window | merge_relocalization | landmark_csr | split_chunks | count_entries | assign_groups | write_lists | layout_blob, layout_workspace | fill_values, write_tables
// UVS_PACK_PROFILE=1 prints a lap per stage on stderr, UVS_DEBUG_LISTS=1 the list lengths of every gather group.
#include "uvs_pack.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace uvspack {

static inline int rup(int v, int m) { return (v + m - 1) / m * m; }

int validate_window(const uvs_window* w, std::string& err) {
    if (!w) { err = "null window"; return UVS_ERR_INVALID_ARG; }
    if (w->n_points < 0 || w->n_point_obs < 0 || w->n_lines < 0 || w->n_line_obs < 0 || w->n_imu < 0 || w->n_imu > UVS_WINDOW_SIZE) { err = "bad counts"; return UVS_ERR_INVALID_ARG; }
    if ((w->n_point_obs && (!w->pt_lm || !w->pt_fi || !w->pt_fj || !w->pt_pi || !w->pt_pj || !w->inv_depth)) ||
        (w->n_line_obs && (!w->ln_lm || !w->ln_fj || !w->ln_sp || !w->ln_ep || !w->ln_has_vp || !w->ln_vp || !w->line_orth)) || (w->n_imu && !w->imu)) { err = "null array"; return UVS_ERR_INVALID_ARG; }
    int prev = -1, prev_fj = -1, anchor = -1;
    for (int k = 0; k < w->n_point_obs; ++k) {
        const int lm = w->pt_lm[k], fi = w->pt_fi[k], fj = w->pt_fj[k];
        if (lm < 0 || lm >= w->n_points || lm < prev) { err = "point observations must be grouped by non-decreasing landmark index"; return UVS_ERR_INVALID_ARG; }
        if (fi < 0 || fj <= fi || fj >= UVS_NUM_FRAMES) { err = "point observation needs 0 <= imu_i < imu_j <= WINDOW_SIZE"; return UVS_ERR_INVALID_ARG; }
        if (lm != prev) { anchor = fi; prev_fj = -1; }
        if (fi != anchor || fj <= prev_fj) { err = "point observations of one landmark must share imu_i and have increasing imu_j"; return UVS_ERR_INVALID_ARG; }
        prev = lm; prev_fj = fj;
    }
    prev = -1; prev_fj = -1;
    for (int k = 0; k < w->n_line_obs; ++k) {
        const int lm = w->ln_lm[k], fj = w->ln_fj[k];
        if (lm < 0 || lm >= w->n_lines || lm < prev) { err = "line observations must be grouped by non-decreasing landmark index"; return UVS_ERR_INVALID_ARG; }
        if (fj < 0 || fj >= UVS_NUM_FRAMES) { err = "line observation frame out of range"; return UVS_ERR_INVALID_ARG; }
        if (lm != prev) prev_fj = -1;
        if (fj <= prev_fj) { err = "line observations of one landmark must have increasing imu_j"; return UVS_ERR_INVALID_ARG; }
        prev = lm; prev_fj = fj;
    }
    for (int b = 0; b < w->n_imu; ++b) if (w->imu[b].frame_i < 0 || w->imu[b].frame_i >= UVS_WINDOW_SIZE) { err = "imu frame_i out of range"; return UVS_ERR_INVALID_ARG; }
    // the prior's block table is checked HERE only: every packing path runs this function before it reads the table (a structure-cache hit does not, but a hit
    // means the table equals, field by field, one that passed: PackCache::matches)
    if (w->prior && w->prior->n > 0) {
        const uvs_prior& p = *w->prior;
        if (p.n > UVS_MAX_PRIOR_DIM || p.n_blocks < 1 || p.n_blocks > UVS_MAX_PRIOR_BLOCKS) { err = "prior too large"; return UVS_ERR_CAPACITY; }
        if (!p.linearized_jacobians || !p.linearized_residuals || !p.x0) { err = "null array"; return UVS_ERR_INVALID_ARG; }
        for (int b = 0; b < p.n_blocks; ++b) {
            // kind <-> global size: pose / extrinsic 7, speed-bias 9, time offset 1; x0_off addresses x0[UVS_PRIOR_X0_LEN]
            const int kind = p.block_kind[b], want = kind == UVS_BLOCK_SPEEDBIAS ? 9 : kind == UVS_BLOCK_TD ? 1 : 7;
            if (kind < UVS_BLOCK_POSE || kind > UVS_BLOCK_TD || p.block_size[b] != want) { err = "prior block kind / size mismatch"; return UVS_ERR_INVALID_ARG; }
            if (p.x0_off[b] < 0 || p.x0_off[b] > UVS_PRIOR_X0_LEN - p.block_size[b]) { err = "prior x0 offset out of range"; return UVS_ERR_INVALID_ARG; }
            const int loc = p.block_size[b] == 7 ? 6 : p.block_size[b];
            if (p.block_idx[b] < 0 || p.block_idx[b] + loc > p.n) { err = "prior block index out of range"; return UVS_ERR_INVALID_ARG; }
            if ((p.block_kind[b] == UVS_BLOCK_POSE || p.block_kind[b] == UVS_BLOCK_SPEEDBIAS) && (p.block_frame[b] < 0 || p.block_frame[b] >= UVS_NUM_FRAMES)) { err = "prior frame out of range"; return UVS_ERR_INVALID_ARG; }
            // every kept block once, every prior column once: two blocks on the same parameter block would map two prior columns to one index of the reduced system, and the
            // device's (H0 entry, S offset) table -- generated with one slot per pair of S indices -- would be overrun (setup_window)
            for (int a = 0; a < b; ++a) {
                const int loca = p.block_size[a] == 7 ? 6 : p.block_size[a];
                const bool same_block = p.block_kind[a] == kind && (kind == UVS_BLOCK_EX_POSE || kind == UVS_BLOCK_TD || p.block_frame[a] == p.block_frame[b]);
                const bool overlap = p.block_idx[a] < p.block_idx[b] + loc && p.block_idx[b] < p.block_idx[a] + loca;
                if (same_block || overlap) { err = "prior keeps a parameter block twice / its blocks overlap"; return UVS_ERR_INVALID_ARG; }
            }
        }
    }
    return UVS_OK;
}

int pack_threads(unsigned most, unsigned share) {
    const char* env = std::getenv("UVS_PACK_THREADS");
    return std::max(1, env ? std::atoi(env) : (int)std::min<unsigned>(most, std::max(1u, std::thread::hardware_concurrency() / share)));
}
int pack_inner_threads(int n_obs) { return n_obs < kPackCacheMinObs ? 1 : pack_threads(8u, 1u); }

bool PackCache::matches(const uvs_window* w, const uvs_options& o, int grid, bool all) const {
    if (!valid || !w || grid != chunk_grid || all != all_blocks || (o.estimate_td != 0) != (td_on != 0) || (o.estimate_extrinsic != 0) != (ex_on != 0) || w->n_relo_obs > 0) return false;
    if (w->n_points != n_points || w->n_point_obs != n_pt_obs || w->n_lines != n_lines || w->n_line_obs != n_ln_obs || w->n_imu != n_imu) return false;
    const bool hp = w->prior && w->prior->n > 0;
    if (hp != have_prior) return false;
    if (hp) {
        const uvs_prior& p = *w->prior;
        if (p.n != prior_n || p.n_blocks != prior_nb || p.n_blocks > UVS_MAX_PRIOR_BLOCKS) return false;
        for (int b = 0; b < p.n_blocks; ++b) if (p.block_kind[b] != prior_tab[0][b] || p.block_frame[b] != prior_tab[1][b] || p.block_size[b] != prior_tab[2][b] || p.block_idx[b] != prior_tab[3][b] || p.x0_off[b] != prior_tab[4][b]) return false;
        if (!p.linearized_jacobians || !p.linearized_residuals || !p.x0) return false;
    }
    if ((n_pt_obs && (!w->pt_lm || !w->pt_fi || !w->pt_fj || !w->pt_pi || !w->pt_pj || !w->inv_depth)) || (n_ln_obs && (!w->ln_lm || !w->ln_fj || !w->ln_sp || !w->ln_ep || !w->ln_has_vp || !w->ln_vp || !w->line_orth)) || (n_imu && !w->imu)) return false;
    if (td_on && n_pt_obs && (!w->pt_vel_i || !w->pt_vel_j || !w->pt_td_i || !w->pt_td_j)) return false;
    for (int b = 0; b < n_imu; ++b) if (w->imu[b].frame_i != imu_fs[b][0] || (w->imu[b].skip ? 1 : 0) != imu_fs[b][1]) return false;
    const size_t np_ = (size_t)n_pt_obs * 4, nl_ = (size_t)n_ln_obs * 4;
    return (!np_ || (!std::memcmp(w->pt_lm, pt_lm.data(), np_) && !std::memcmp(w->pt_fi, pt_fi.data(), np_) && !std::memcmp(w->pt_fj, pt_fj.data(), np_))) &&
           (!nl_ || (!std::memcmp(w->ln_lm, ln_lm.data(), nl_) && !std::memcmp(w->ln_fj, ln_fj.data(), nl_) && !std::memcmp(w->ln_has_vp, ln_has_vp.data(), nl_)));
}
void PackCache::store(const uvs_window* w, const uvs_options& o, int grid, bool all, const DevWin& h) {
    valid = true; device_holds_tables = false; chunk_grid = grid; all_blocks = all; td_on = o.estimate_td != 0; ex_on = o.estimate_extrinsic != 0;
    n_points = w->n_points; n_pt_obs = w->n_point_obs; n_lines = w->n_lines; n_ln_obs = w->n_line_obs; n_imu = w->n_imu;
    pt_lm.assign(w->pt_lm, w->pt_lm + n_pt_obs); pt_fi.assign(w->pt_fi, w->pt_fi + n_pt_obs); pt_fj.assign(w->pt_fj, w->pt_fj + n_pt_obs);
    ln_lm.assign(w->ln_lm, w->ln_lm + n_ln_obs); ln_fj.assign(w->ln_fj, w->ln_fj + n_ln_obs); ln_has_vp.assign(w->ln_has_vp, w->ln_has_vp + n_ln_obs);
    for (int b = 0; b < n_imu; ++b) { imu_fs[b][0] = w->imu[b].frame_i; imu_fs[b][1] = w->imu[b].skip ? 1 : 0; }
    have_prior = w->prior && w->prior->n > 0;
    if (have_prior) { const uvs_prior& p = *w->prior; prior_n = p.n; prior_nb = p.n_blocks; for (int b = 0; b < p.n_blocks; ++b) { prior_tab[0][b] = p.block_kind[b]; prior_tab[1][b] = p.block_frame[b]; prior_tab[2][b] = p.block_size[b]; prior_tab[3][b] = p.block_idx[b]; prior_tab[4][b] = p.x0_off[b]; } }
    hdr = h;
}

void fill_values(char* B, const DevWin& h, const uvs_window* w, bool td_on, int threads) {
    double* D = (double*)B;
    std::memcpy(B, &h, sizeof(h));
    std::memcpy(D + h.d_frames, w->pose, sizeof(double) * 77);
    std::memcpy(D + h.d_frames + 77, w->speedbias, sizeof(double) * 99);
    std::memcpy(D + h.d_frames + 176, w->ex_pose, sizeof(double) * 7);
    D[h.d_frames + 183] = w->td;
    std::memcpy(D + h.d_frames + 184, w->relo_pose, sizeof(double) * 7);
    for (int k = 0; k < h.n_points; ++k) D[h.d_invd + k] = w->inv_depth[k];
    pack_parallel(h.n_pt_obs, threads, [&](int k0_, int k1_, int) {
        for (int k = k0_; k < k1_; ++k) {
            for (int q = 0; q < 3; ++q) { D[h.d_ptmeas + q * h.pt_stride + k] = w->pt_pi[3 * k + q]; D[h.d_ptmeas + (3 + q) * h.pt_stride + k] = w->pt_pj[3 * k + q]; }
            if (td_on) {
                for (int q = 0; q < 2; ++q) { D[h.d_ptvel + q * h.pt_stride + k] = w->pt_vel_i[2 * k + q]; D[h.d_ptvel + (2 + q) * h.pt_stride + k] = w->pt_vel_j[2 * k + q]; }
                D[h.d_ptvel + 4 * h.pt_stride + k] = w->pt_td_i[k]; D[h.d_ptvel + 5 * h.pt_stride + k] = w->pt_td_j[k];
            }
        }
    });
    for (int k = 0; k < 4 * h.n_lines; ++k) D[h.d_line + k] = w->line_orth[k];
    pack_parallel(h.n_ln_obs, threads, [&](int k0_, int k1_, int) {
        for (int k = k0_; k < k1_; ++k)
            for (int q = 0; q < 3; ++q) {
                D[h.d_lnmeas + q * h.ln_stride + k] = w->ln_sp[3 * k + q]; D[h.d_lnmeas + (3 + q) * h.ln_stride + k] = w->ln_ep[3 * k + q];
                D[h.d_lnmeas + (6 + q) * h.ln_stride + k] = w->ln_vp[3 * k + q];
            }
    });
    for (int b = 0; b < h.n_imu; ++b) {
        const uvs_imu_block& ib = w->imu[b];
        double* blk = D + h.d_imu + (size_t)b * UVS_IMU_STRIDE;
        blk[0] = ib.sum_dt;
        for (int q = 0; q < 3; ++q) { blk[1 + q] = ib.delta_p[q]; blk[8 + q] = ib.delta_v[q]; blk[11 + q] = ib.linearized_ba[q]; blk[14 + q] = ib.linearized_bg[q]; }
        for (int q = 0; q < 4; ++q) blk[4 + q] = ib.delta_q[q];
        {   // only the five 3x3 blocks the factor reads, packed (UVS_IMU_JIDX)
            const int RC[5][2] = {{0, 9}, {0, 12}, {3, 12}, {6, 9}, {6, 12}};
            for (int q = 0; q < 5; ++q) for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) blk[UVS_IMU_JAC + 9 * q + 3 * i + j] = ib.jacobian[(RC[q][0] + i) * 15 + RC[q][1] + j];
        }
        std::memcpy(blk + UVS_IMU_COV, ib.covariance, sizeof(double) * 225);
    }
    if (h.prior_n > 0) {
        const uvs_prior& p = *w->prior;
        const int n = p.n;
        std::memcpy(D + h.d_prior, p.linearized_jacobians, sizeof(double) * (size_t)n * n);      // row-major, read once per solve (setup_window builds J0^T J0, J0^T r0 from it)
        for (int r = 0; r < n; ++r) D[h.d_prior + n * n + r] = p.linearized_residuals[r];
        // linearization point of block b at stride 9 (not at x0_off[b]): the kernel's loads of it then do not depend on a table load
        for (int b = 0; b < p.n_blocks && b < 16; ++b) for (int k = 0; k < p.block_size[b] && k < 9; ++k) D[h.d_prior + n * n + 2 * n + 9 * b + k] = p.x0[p.x0_off[b] + k];
    }
}

namespace {

constexpr int NG = UVS_NGRP, GPW = UVS_GRP_PER_WAVE, NW = UVS_GWAVES;      // gather groups (UVS_GLANES lanes each), per wave, and the waves that hold them
constexpr long kStageCap = (long)UVS_S_DOUBLES;                           // the LDS staging area a chunk must fit
constexpr long kListHdr = 2 * (NG + 1);                                   // ints ahead of a chunk's entries: schur_off[NG + 1] direct_off[NG + 1]

// What pack_window's stages hand one another (all of it locals of one 520-line function once).  The vectors are the ones that function had; the
// per-block and per-group tables are plain arrays: a batch packs 256 small windows per call, and a plan must not allocate more than the locals did.
struct PackPlan {
    const uvs_window* w = nullptr;      // the window as packed: the caller's, or `merged` (relocalization blocks among the point observations)
    uvs_window merged;
    std::vector<int32_t> m_lm, m_fi, m_fj, eidx; std::vector<double> m_pi, m_pj, m_vi, m_vj, m_tdi, m_tdj;      // the arrays `merged` points to; eidx: merged -> caller's observation
    bool td_on = false, ex_on = false, relo_on = false, relo2 = false, have_prior = false, all_blocks = false;
    int chunk_grid = 0, threads = 1;
    DevWin h;
    std::vector<int> pbeg, lbeg;        // CSR begins by landmark
    std::vector<int> chunks;            // UVS_CHUNK_INTS ints per chunk (uvs_layout.h: i_chunks)
    std::vector<int> cnt_s, cnt_d;      // entries per chunk and pose block (first pass), reused when the lists are written
    long blk_s[UVS_NBLKX2], blk_d[UVS_NBLKX2], blk_wp[UVS_NBLKX2], blk_wl[UVS_NBLKX2];      // work per pose block: Schur, direct; in the point chunks, in the line chunks
    int wblk[NG], g_blk[NG], g_part[NG], g_np[NG];      // gather group -> i_wblk word; block, part, parts of its block
    std::vector<int> lists;             // i_lists
    int pblk[UVS_NBLK], n_pblk = 0;     // S blocks the prior touches
    int n_chunks() const { return (int)chunks.size() / UVS_CHUNK_INTS; }
};

// LDS doubles the records and Schur factors of `nob` observations of `nlm` landmarks occupy (type 0: points, 1: lines) -- also the measure of a whole family's
// share of the work -- and with the gather lists (ints, 2 per double) on top: what a chunk needs.  The estimate that cuts the chunks, its lower bound and
// the check of the lists actually written all use these two.
inline long family_doubles(const DevWin& h, int type, long nob, long nlm) {
    return type == 0 ? (long)h.pt_rec * nob + 12 * (nob + h.pt_xslots * nlm) : (long)(UVS_LN_REC + 2 * UVS_LN_EY) * nob + 20 * nlm;
}
inline long chunk_doubles(const DevWin& h, int type, long nob, long nlm, long list_ints) { return family_doubles(h, type, nob, nlm) + (list_ints + 1) / 2; }

// index in the reduced system S of dof q of the prior's block b; -1: the column is dropped (a constant Ex_Pose -- ESTIMATE_EXTRINSIC == 0 -- drops its columns,
// SURVEY.md Appendix B.1; a free one maps dof q to the spare slot of frame q)
inline int prior_s_index(const uvs_prior& p, int b, int q, bool td_on, bool ex_on) {
    switch (p.block_kind[b]) {
        case UVS_BLOCK_POSE: return 16 * p.block_frame[b] + q;
        case UVS_BLOCK_SPEEDBIAS: return 16 * p.block_frame[b] + 6 + q;
        case UVS_BLOCK_TD: return td_on ? UVS_TD_INDEX + q : -1;
        case UVS_BLOCK_EX_POSE: return ex_on ? UVS_EX_INDEX(q) : -1;
    }
    return -1;
}
inline int prior_block_dofs(const uvs_prior& p, int b) { return p.block_size[b] == 7 ? 6 : p.block_size[b]; }

// Relocalization blocks (estimator.cpp:944-978) become ordinary point observations whose second frame is the pseudo frame 12 = relo_Pose,
// placed right after their landmark's last observation (the kernel wants a landmark's blocks together).  eidx maps a merged observation
// back to the caller's index (-1 for a relocalization block): uvs_evaluate / uvs_marginalize keep the caller's numbering and skip them.
int merge_relocalization(const uvs_window* w_in, PackPlan& P, std::string& err) {
    // relo_Pose takes the six spare slots of the reduced system that a free extrinsic would take; the time offset has its own (index 175), so
    // ESTIMATE_TD and relocalization blocks coexist (estimator.cpp:784-797 + :944-978)
    // with a free extrinsic the spare slots are taken: relo_Pose becomes a second-level block (uvs_layout.h: UVS_RELO2_BLOCKROW) -- in the persistent kernel and, since
    // round 6, in the landmark-sharded forms of one rank (chunk_grid > 0; uvs_large_kernel.h: LG_R2)
    const int n_relo = w_in->n_relo_obs; const bool td_on = P.td_on;
    auto &m_lm = P.m_lm, &m_fi = P.m_fi, &m_fj = P.m_fj, &eidx = P.eidx; auto &m_pi = P.m_pi, &m_pj = P.m_pj, &m_vi = P.m_vi, &m_vj = P.m_vj, &m_tdi = P.m_tdi, &m_tdj = P.m_tdj;
    if (!w_in->relo_lm || !w_in->relo_pi || !w_in->relo_pj) { err = "null array"; return UVS_ERR_INVALID_ARG; }
    const int npo = w_in->n_point_obs;
    int q = 0;
    for (int k = 0; k < npo; ++k) {
        const int lm = w_in->pt_lm[k];
        m_lm.push_back(lm); m_fi.push_back(w_in->pt_fi[k]); m_fj.push_back(w_in->pt_fj[k]); eidx.push_back(k);
        for (int c = 0; c < 3; ++c) { m_pi.push_back(w_in->pt_pi[3 * k + c]); m_pj.push_back(w_in->pt_pj[3 * k + c]); }
        if (td_on) { for (int c = 0; c < 2; ++c) { m_vi.push_back(w_in->pt_vel_i[2 * k + c]); m_vj.push_back(w_in->pt_vel_j[2 * k + c]); } m_tdi.push_back(w_in->pt_td_i[k]); m_tdj.push_back(w_in->pt_td_j[k]); }
        if (k + 1 < npo && w_in->pt_lm[k + 1] == lm) continue;
        if (q < n_relo && w_in->relo_lm[q] < lm) { err = "relo_lm must be strictly increasing and name landmarks that have observations"; return UVS_ERR_INVALID_ARG; }
        if (q < n_relo && w_in->relo_lm[q] == lm) {
            m_lm.push_back(lm); m_fi.push_back(w_in->pt_fi[k]); m_fj.push_back(UVS_RELO_FRAME); eidx.push_back(-1);
            for (int c = 0; c < 3; ++c) { m_pi.push_back(w_in->relo_pi[3 * q + c]); m_pj.push_back(w_in->relo_pj[3 * q + c]); }
            // a relocalization block is the plain ProjectionFactor also under ESTIMATE_TD (estimator.cpp:967-970): zero image velocities
            // switch the time-offset terms of its record off (no shift of pts_i / pts_j, d r / d td = 0)
            if (td_on) { for (int c = 0; c < 2; ++c) { m_vi.push_back(0.0); m_vj.push_back(0.0); } m_tdi.push_back(w_in->td); m_tdj.push_back(w_in->td); }
            ++q;
        }
    }
    if (q != n_relo) { err = "relo_lm must be strictly increasing and name landmarks that have observations"; return UVS_ERR_INVALID_ARG; }
    uvs_window& wm = P.merged;
    wm = *w_in;
    wm.n_point_obs = (int)m_lm.size(); wm.pt_lm = m_lm.data(); wm.pt_fi = m_fi.data(); wm.pt_fj = m_fj.data(); wm.pt_pi = m_pi.data(); wm.pt_pj = m_pj.data();
    if (td_on) { wm.pt_vel_i = m_vi.data(); wm.pt_vel_j = m_vj.data(); wm.pt_td_i = m_tdi.data(); wm.pt_td_j = m_tdj.data(); }
    P.w = &wm;
    return UVS_OK;
}

// counts and options of the header: what every later stage reads from P.h
void start_header(PackPlan& P, int n_relo) {
    DevWin& h = P.h; const uvs_window* w = P.w;
    std::memset(&h, 0, sizeof(h));
    h.n_points = w->n_points; h.n_pt_obs = w->n_point_obs; h.n_lines = w->n_lines; h.n_ln_obs = w->n_line_obs; h.n_imu = w->n_imu;
    P.have_prior = w->prior && w->prior->n > 0;
    h.prior_n = P.have_prior ? w->prior->n : 0; h.prior_nb = P.have_prior ? w->prior->n_blocks : 0;
    h.pt_stride = rup(std::max(h.n_pt_obs, 1), 8); h.ln_stride = rup(std::max(h.n_ln_obs, 1), 8);
    h.td_on = P.td_on ? 1 : 0; h.ex_on = P.ex_on ? 1 : 0;
    P.relo_on = n_relo > 0;
    h.relo_on = P.relo_on ? 1 : 0; h.n_relo = n_relo;
    P.relo2 = P.relo_on && P.ex_on;      // relo_Pose as a second-level block (block row 13 of the gather)
    h.relo2 = P.relo2 ? 1 : 0;
    h.pt_rec = P.ex_on ? UVS_PT_REC_EX : P.td_on ? UVS_PT_REC_TD : UVS_PT_REC; h.pt_xslots = 1 + (P.td_on ? 1 : 0) + (P.ex_on ? 1 : 0);
    h.n_parts = 1;
}

// CSR by landmark
void landmark_csr(PackPlan& P) {
    const DevWin& h = P.h; const uvs_window* w = P.w;
    P.pbeg.assign(h.n_points + 1, 0); P.lbeg.assign(h.n_lines + 1, 0);
    for (int k = 0; k < h.n_pt_obs; ++k) P.pbeg[w->pt_lm[k] + 1]++;
    for (int k = 0; k < h.n_points; ++k) P.pbeg[k + 1] += P.pbeg[k];
    for (int k = 0; k < h.n_ln_obs; ++k) P.lbeg[w->ln_lm[k] + 1]++;
    for (int k = 0; k < h.n_lines; ++k) P.lbeg[k + 1] += P.lbeg[k];
}

// chunks: greedy packing of whole landmarks into the LDS staging area (UVS_S_DOUBLES doubles).  A chunk holds the
// observation records, the per-landmark Schur factors AND its gather lists (ints, 2 per double).
int split_chunks(PackPlan& P, std::string& err) {
    const DevWin& h = P.h; const bool td_on = P.td_on, ex_on = P.ex_on; const int XS = h.pt_xslots, chunk_grid = P.chunk_grid;
    const std::vector<int>&pbeg = P.pbeg, &lbeg = P.lbeg;
    // LDS doubles a chunk of landmarks [k0, k1) needs (records + Schur factors + gather lists), -1 if an index field overflows
    auto need_pt = [&](int k0, int k1) -> long {
        long nob = pbeg[k1] - pbeg[k0], nlm = k1 - k0, nli = kListHdr;
        // Schur entries: all slot pairs of the landmark; direct entries per observation: 3, + 3 with td, + 3 with ex (+ 1 more with both: (ex, td))
        const long dper = 3 + (td_on ? 3 : 0) + (ex_on ? 3 + (td_on ? 1 : 0) : 0);
        for (int k = k0; k < k1; ++k) { const long no = pbeg[k + 1] - pbeg[k]; nli += no ? (no + XS) * (no + XS + 1) / 2 + dper * no : 0; }
        if (nlm > 1023 || nob + XS * nlm > 16383) return -1;
        return chunk_doubles(h, 0, nob, nlm, nli);
    };
    auto need_ln = [&](int k0, int k1) -> long {
        long nob = lbeg[k1] - lbeg[k0], nlm = k1 - k0, nli = kListHdr;
        for (int k = k0; k < k1; ++k) { const long no = lbeg[k + 1] - lbeg[k]; nli += no * (no + 1) / 2 + no; }
        if (nlm > 1023 || nob > 16383) return -1;
        return chunk_doubles(h, 1, nob, nlm, nli);
    };
    // even split (by observation count) of a landmark family into n chunks; empty vector if some chunk does not fit the staging area
    auto cuts_for = [&](int n, int n_lm, const std::vector<int>& beg, auto&& need) -> std::vector<int> {
        std::vector<int> cut(1, 0);
        const long tot = beg[n_lm];
        for (int j = 1; j < n; ++j) {
            int k = cut.back() + 1;
            while (k < n_lm && (long)beg[k] * n < tot * j) ++k;
            cut.push_back(std::min(k, n_lm - (n - j)));
        }
        cut.push_back(n_lm);
        for (int j = 0; j < n; ++j) { const long nd = need(cut[j], cut[j + 1]); if (!(cut[j + 1] > cut[j] && nd >= 0 && nd <= kStageCap)) return {}; }
        return cut;
    };
    // smallest number of chunks >= n_from whose even split fits; the kernel pays a fixed cost per chunk, so a greedy fill that leaves a
    // nearly empty last chunk would waste a whole pass
    auto split = [&](int type, int n_lm, const std::vector<int>& beg, auto&& need, int n_from, std::vector<int>& cut) -> int {
        cut.clear();
        if (n_lm == 0) return UVS_OK;
        // start at the capacity lower bound (records + Schur factors alone; the lists come on top): walking n = 1, 2, ... costs
        // O(n * landmarks) per attempt, milliseconds for the 340 chunks of configs[3]
        const long mine = type == 0 ? family_doubles(h, 0, h.n_pt_obs, h.n_points) : family_doubles(h, 1, h.n_ln_obs, h.n_lines);
        const int n_first = (int)std::min<long>(n_lm, std::max<long>(std::max(1, n_from), mine / kStageCap));
        for (int n = n_first; n <= n_lm; ++n) { cut = cuts_for(n, n_lm, beg, need); if (!cut.empty()) return UVS_OK; }
        return UVS_ERR_CAPACITY;
    };
    std::vector<int> cut_pt, cut_ln;
    if (split(0, h.n_points, pbeg, need_pt, 1, cut_pt) != UVS_OK) { err = "single point landmark exceeds LDS staging"; return UVS_ERR_CAPACITY; }
    if (split(1, h.n_lines, lbeg, need_ln, 1, cut_ln) != UVS_OK) { err = "single line landmark exceeds LDS staging"; return UVS_ERR_CAPACITY; }
    if (chunk_grid > 0) {
        const int n_pt = cut_pt.empty() ? 0 : (int)cut_pt.size() - 1, n_ln = cut_ln.empty() ? 0 : (int)cut_ln.size() - 1, n_min = n_pt + n_ln;
        // work per family ~ its staging volume; a chunk should keep at least ~64 observations (its fixed cost is a few microseconds)
        const double w_pt = (double)family_doubles(h, 0, h.n_pt_obs, h.n_points), w_ln = (double)family_doubles(h, 1, h.n_ln_obs, h.n_lines);
        static const long min_obs = std::getenv("UVS_CHUNK_MIN_OBS") ? std::max(1, std::atoi(std::getenv("UVS_CHUNK_MIN_OBS"))) : 64;
        const long by_size = (long)(h.n_pt_obs + h.n_ln_obs) / min_obs;
        long target = n_min >= chunk_grid ? (long)((n_min + chunk_grid - 1) / chunk_grid) * chunk_grid : std::min<long>(chunk_grid, std::max<long>(n_min, by_size));
        if (target > n_min && w_pt + w_ln > 0.0) {
            int t_pt = (int)std::lround(target * w_pt / (w_pt + w_ln));
            t_pt = std::max(n_pt, std::min(t_pt, (int)target - n_ln));
            int t_ln = (int)target - t_pt;
            t_pt = std::min(t_pt, h.n_points); t_ln = std::min(t_ln, h.n_lines);
            std::vector<int> c2;
            if (t_pt > n_pt && split(0, h.n_points, pbeg, need_pt, t_pt, c2) == UVS_OK) cut_pt = c2;
            if (t_ln > n_ln && split(1, h.n_lines, lbeg, need_ln, t_ln, c2) == UVS_OK) cut_ln = c2;
        }
    }
    std::vector<int>& chunks = P.chunks;
    for (size_t j = 0; j + 1 < cut_pt.size(); ++j) chunks.insert(chunks.end(), {0, cut_pt[j], cut_pt[j + 1], 0, 0, 0, pbeg[cut_pt[j]], pbeg[cut_pt[j + 1]] - pbeg[cut_pt[j]]});
    for (size_t j = 0; j + 1 < cut_ln.size(); ++j) chunks.insert(chunks.end(), {1, cut_ln[j], cut_ln[j + 1], 0, 0, 0, lbeg[cut_ln[j]], lbeg[cut_ln[j + 1]] - lbeg[cut_ln[j]]});
    return UVS_OK;
}

// gather lists per chunk and per lower 6x6 pose block (see uvs_solve_kernel.h: gather_points / gather_lines),
// pre-expanded into LDS offsets (doubles from the staging base; the chunk layout below mirrors lin_chunk()):
//   points: rec[nob][30] | E[(nob+nlm)][6] | EI[(nob+nlm)][6] | lists      lines: rec[nob][34] | E[nob][24] | Y[nob][24] | X[nlm][20] | lists
//   Schur entry : offset(E row of frame a) | offset(EI / Y row of frame b) << 16
//   direct entry: points: offset(first Jacobian block) | offset(second) << 16   (A^T A, B^T B, B^T A) ; lines: record offset
// The generator of one chunk's entries: addS(block, entry) for every Schur entry, addD(block, entry) for every direct one, each block's in a fixed order.
// Two passes run it: the first only COUNTS the entries per pose block (what the work split needs), the second regenerates them chunk by chunk
// while the lists are written.  (Keeping every chunk's entries alive between the passes cost 80 k small vectors on a configs[3]-sized window:
// two thirds of the packing time.)
struct ChunkEntries {
    const int* chunks; const int* pbeg; const int* lbeg; const uvs_window* w; int PREC, XS; bool td_on, ex_on, relo2;
    explicit ChunkEntries(const PackPlan& P) : chunks(P.chunks.data()), pbeg(P.pbeg.data()), lbeg(P.lbeg.data()), w(P.w), PREC(P.h.pt_rec), XS(P.h.pt_xslots), td_on(P.td_on), ex_on(P.ex_on), relo2(P.relo2) {}
    static int blk_of(int fa, int fb) { return fa * (fa + 1) / 2 + fb; }   // fa >= fb ; fa == 11 is the time-offset pseudo frame: 66 + fb
    template <class S, class D> void operator()(int qc, S&& addS, D&& addD) const {
        const int type = chunks[UVS_CHUNK_INTS * qc], k0 = chunks[UVS_CHUNK_INTS * qc + 1], k1 = chunks[UVS_CHUNK_INTS * qc + 2];
        if (type == 0) {
            const int o0 = pbeg[k0], nob = pbeg[k1] - o0, nlm = k1 - k0;
            const int oE = nob * PREC, oEI = oE + 6 * (nob + XS * nlm);
            for (int k = k0; k < k1; ++k) {
                const int li = k - k0, b0 = pbeg[k] - o0, b1 = pbeg[k + 1] - o0;
                if (b1 == b0) continue;
                const int first_slot = b0 + XS * li;
                int fr[UVS_NUM_FRAMES + 4], nf = 0;      // block rows of the landmark's Schur slots
                fr[nf++] = w->pt_fi[o0 + b0];
                for (int o = b0; o < b1; ++o) fr[nf++] = (relo2 && w->pt_fj[o0 + o] == UVS_RELO_FRAME) ? UVS_RELO2_BLOCKROW : w->pt_fj[o0 + o];
                if (td_on) fr[nf++] = UVS_NUM_FRAMES;                                  // then the td slot of this landmark (pseudo frame 11)
                if (ex_on) fr[nf++] = UVS_NUM_FRAMES + 1;                              // then its extrinsic slot (pseudo frame 12)
                for (int sa = 0; sa < nf; ++sa) for (int sb = 0; sb <= sa; ++sb) {    // frames increase with the slot, except a relocalization block (pseudo frame 12) ahead of the td slot (11)
                    const bool up = fr[sa] >= fr[sb];
                    const int ra = up ? sa : sb, rb = up ? sb : sa;
                    addS(blk_of(fr[ra], fr[rb]), (oE + 6 * (first_slot + ra)) | ((oEI + 6 * (first_slot + rb)) << 16));
                }
                for (int o = b0; o < b1; ++o) {
                    const bool is_relo = w->pt_fj[o0 + o] == UVS_RELO_FRAME;
                    const int fi = w->pt_fi[o0 + o], fj = (relo2 && is_relo) ? UVS_RELO2_BLOCKROW : w->pt_fj[o0 + o], ro = o * PREC;
                    addD(blk_of(fi, fi), (ro + UVS_PT_A) | UVS_PT_ENTRY_A | ((ro + UVS_PT_A) << 16));      // (flag: this entry's corrected residual sits 26, not 12, doubles behind its first operand)
                    addD(blk_of(fj, fj), (ro + UVS_PT_B) | ((ro + UVS_PT_B) << 16));
                    addD(blk_of(fj, fi), (ro + UVS_PT_B) | ((ro + UVS_PT_A) << 16));
                    if (td_on && !is_relo) {                                           // J_td^T [A | B | J_td]  (a relocalization block does not depend on td)
                        addD(blk_of(UVS_NUM_FRAMES, fi), (ro + UVS_PT_TD) | ((ro + UVS_PT_A) << 16));
                        addD(blk_of(UVS_NUM_FRAMES, fj), (ro + UVS_PT_TD) | ((ro + UVS_PT_B) << 16));
                        addD(blk_of(UVS_NUM_FRAMES, UVS_NUM_FRAMES), (ro + UVS_PT_TD) | ((ro + UVS_PT_TD) << 16));
                    }
                    if (ex_on) {                                                       // J_ex^T [A | B | J_td | J_ex]
                        const int X = UVS_NUM_FRAMES + 1;
                        addD(blk_of(X, fi), (ro + UVS_PT_EX) | ((ro + UVS_PT_A) << 16));
                        if (fj > X) addD(blk_of(fj, X), (ro + UVS_PT_B) | ((ro + UVS_PT_EX) << 16));      // (relo_Pose, ex): the rows are relo_Pose's
                        else addD(blk_of(X, fj), (ro + UVS_PT_EX) | ((ro + UVS_PT_B) << 16));
                        if (td_on && !is_relo) addD(blk_of(X, UVS_NUM_FRAMES), (ro + UVS_PT_EX) | ((ro + UVS_PT_TD) << 16));
                        addD(blk_of(X, X), (ro + UVS_PT_EX) | ((ro + UVS_PT_EX) << 16));
                    }
                }
            }
        } else {
            const int o0 = lbeg[k0], nob = lbeg[k1] - o0;
            const int oE = nob * UVS_LN_REC, oY = oE + UVS_LN_EY * nob;
            for (int k = k0; k < k1; ++k) {
                const int b0 = lbeg[k] - o0, b1 = lbeg[k + 1] - o0;
                for (int sa = 0; sa < b1 - b0; ++sa) for (int sb = 0; sb <= sa; ++sb)
                    addS(blk_of(w->ln_fj[o0 + b0 + sa], w->ln_fj[o0 + b0 + sb]), (oE + UVS_LN_EY * (b0 + sa)) | ((oY + UVS_LN_EY * (b0 + sb)) << 16));
                for (int o = b0; o < b1; ++o) addD(blk_of(w->ln_fj[o0 + o], w->ln_fj[o0 + o]), o * UVS_LN_REC);
            }
        }
    }
};

// first pass: entries per chunk and pose block, and the work per block and landmark family
void count_entries(PackPlan& P, const ChunkEntries& chunk_entries) {
    const int n_ch = P.n_chunks();
    P.cnt_s.resize((size_t)n_ch * UVS_NBLKX2); P.cnt_d.resize((size_t)n_ch * UVS_NBLKX2);
    struct Cnt { long s[UVS_NBLKX2], d[UVS_NBLKX2], wp[UVS_NBLKX2], wl[UVS_NBLKX2]; };
    std::vector<Cnt> part((size_t)std::max(P.threads, 1));
    for (auto& c : part) std::memset(&c, 0, sizeof(c));
    pack_parallel(n_ch, P.threads, [&](int q0, int q1, int t) {
        Cnt& c = part[t];
        for (int qc = q0; qc < q1; ++qc) {
            long cs[UVS_NBLKX2] = {0}, cd[UVS_NBLKX2] = {0};
            chunk_entries(qc, [&](int b, int) { ++cs[b]; }, [&](int b, int) { ++cd[b]; });
            for (int b = 0; b < UVS_NBLKX2; ++b) { P.cnt_s[(size_t)qc * UVS_NBLKX2 + b] = (int)cs[b]; P.cnt_d[(size_t)qc * UVS_NBLKX2 + b] = (int)cd[b]; }
            const int type = P.chunks[UVS_CHUNK_INTS * qc];
            // work units ~ cycles per entry of the rows-per-lane gather
            for (int b = 0; b < UVS_NBLKX2; ++b) {
                // measured per entry on MI355X (per-wave timers, UVS_DEBUG_GATHER_TIMERS): point Schur 350 cycles, point direct 675 cycles
                const long ws_ = (type == 0 ? 18 : 72) * cs[b], wd_ = (type == 0 ? 35 : 63) * cd[b];
                c.s[b] += ws_; c.d[b] += wd_;
                (type == 0 ? c.wp : c.wl)[b] += ws_ + wd_;      // per landmark family: the chunks of a family are separated by barriers
            }
        }
    });
    for (int b = 0; b < UVS_NBLKX2; ++b) P.blk_s[b] = P.blk_d[b] = P.blk_wp[b] = P.blk_wl[b] = 0;
    for (const auto& c : part) for (int b = 0; b < UVS_NBLKX2; ++b) { P.blk_s[b] += c.s[b]; P.blk_d[b] += c.d[b]; P.blk_wp[b] += c.wp[b]; P.blk_wl[b] += c.wl[b]; }
}

// gather groups: 256 two-lane groups, at least one per pose block; the spare ones split the heaviest blocks further.  Groups are dealt to
// the waves heaviest first (similar list lengths inside a wave => little divergence); the wave order pairs heavy with light
// waves on a SIMD (waves w and w+4 share one).
void assign_groups(PackPlan& P) {
    DevWin& h = P.h; const bool td_on = P.td_on, ex_on = P.ex_on, relo_on = P.relo_on, relo2 = P.relo2, all_blocks = P.all_blocks;
    const long *blk_s = P.blk_s, *blk_d = P.blk_d, *blk_wp = P.blk_wp, *blk_wl = P.blk_wl;
    long blk_work[UVS_NBLKX2];
    for (int b = 0; b < UVS_NBLKX2; ++b) blk_work[b] = blk_s[b] + blk_d[b];
    struct Item { int b, part, np; long work; double shape; };
    // water-filling: hand the spare groups, one at a time, to the block whose per-group share is largest (at most 16 parts)
    int np[UVS_NBLKX2]; int used = 0;
    for (int b = 0; b < UVS_NBLKX2; ++b) {      // the pseudo-frame blocks only exist with their option
        const bool tdb = b >= UVS_NBLK && b < UVS_NBLK + UVS_NF + 1, exb = b >= UVS_NBLK + UVS_NF + 1 && b < UVS_NBLKX;
        // a block nothing contributes to (frames further apart than the longest track, pseudo-frame blocks of an option that is off) gets
        // no group at all: S is zeroed anyway, and its group goes to a heavy block instead (15 of 128 groups for the canonical window).
        // all_blocks (a landmark SHARD of a solve over several ranks): every block of an option that is on keeps a group, because k_large_solve loads the all-reduced
        // vector through the part-0 groups -- a block that only the OTHER ranks' landmarks contribute to would otherwise never reach this rank's reduced system
        const bool r2b = b >= UVS_NBLKX;      // block row 13 (relo_Pose beside a free extrinsic)
        np[b] = ((b < UVS_NBLK || (tdb && td_on) || (!r2b && exb && (ex_on || relo_on) && (td_on || b != UVS_NBLK + UVS_NF + 1 + UVS_NF)) || (r2b && relo2 && (td_on || b != UVS_NBLKX + UVS_NF))) && (all_blocks || blk_work[b] > 0)) ? 1 : 0;
        used += np[b];
    }
    // The waves run in lock step inside a chunk and the chunks of the two landmark families are separated by barriers, so what counts
    // is the LARGEST per-group share within each family, not the per-group total: a block that is heavy in the point chunks only (the
    // diagonal blocks: all the J^T J terms) must be split until its point share matches the others', even if its total looks average.
    // Greedy: the next spare group goes to the family whose current maximum weighs more, and there to the block that holds it.
    int act[UVS_NBLKX2], na = 0;      // the blocks that take part (ascending: the scans below keep the tie-breaking order of a scan over all blocks)
    for (int b = 0; b < UVS_NBLKX2; ++b) if (np[b] > 0) act[na++] = b;
    while (used < NG) {
        int bp = -1, bl = -1;
        double mp = 0.0, ml = 0.0;      // the true maxima include the blocks that cannot be split any further
        for (int q = 0; q < na; ++q) {
            const int b = act[q];
            mp = std::max(mp, (double)blk_wp[b] / np[b]); ml = std::max(ml, (double)blk_wl[b] / np[b]);
            if (np[b] >= 16) continue;
            if (blk_wp[b] > 0 && (bp < 0 || blk_wp[b] * np[bp] > blk_wp[bp] * np[b])) bp = b;
            if (blk_wl[b] > 0 && (bl < 0 || blk_wl[b] * np[bl] > blk_wl[bl] * np[b])) bl = b;
        }
        int best = -1;
        const double sp_ = bp >= 0 ? (double)blk_wp[bp] / np[bp] : -1.0, sl_ = bl >= 0 ? (double)blk_wl[bl] / np[bl] : -1.0;
        if (bp >= 0 && sp_ >= mp && (mp >= ml || bl < 0 || sl_ < ml)) best = bp;
        else if (bl >= 0 && sl_ >= ml) best = bl;
        else if (bp >= 0 && (bl < 0 || sp_ >= sl_)) best = bp;
        else best = bl;
        if (best < 0) break;
        ++np[best]; ++used;
    }
    std::vector<Item> items;
    for (int b = 0; b < UVS_NBLKX2; ++b) for (int q = 0; q < np[b]; ++q) items.push_back({b, q, np[b], blk_work[b] / np[b], blk_work[b] ? (double)blk_d[b] / (double)blk_work[b] : -1.0});
    // a wave runs max(Schur count) + max(direct count) iterations over its 32 groups: deal groups of similar SHAPE (share of
    // direct work) to the same wave, idle groups last
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b2) { return a.shape != b2.shape ? a.shape > b2.shape : a.work > b2.work; });
    int wave_of_rank[NW];
    // (identity: the parts of a split block must sit in CONSECUTIVE groups -- gacc_gather_parts addresses part p at lane + p * UVS_GLANES -- and a block may
    // straddle two ranks; the round-2 order for 8 waves, heavy ranks paired with light ones on a SIMD, broke exactly that: the wrong pose blocks of the 512-thread builds)
    for (int r = 0; r < NW; ++r) wave_of_rank[r] = r;
    h.n_parts = 1;
    for (int b = 0; b < UVS_NBLKX2; ++b) h.n_parts = std::max(h.n_parts, np[b]);
    for (int g = 0; g < NG; ++g) { P.wblk[g] = -1; P.g_blk[g] = -1; P.g_part[g] = 0; P.g_np[g] = 1; }
    for (size_t q = 0; q < items.size(); ++q) {
        const int g = wave_of_rank[q / GPW] * GPW + (int)(q % GPW);
        const int b = items[q].b;
        const int bfa = b >= UVS_NBLKX ? UVS_RELO2_BLOCKROW : b >= UVS_NBLK + UVS_NF + 1 ? UVS_NUM_FRAMES + 1 : b >= UVS_NBLK ? UVS_NUM_FRAMES : (int)((std::sqrt(8.0 * b + 1.0) - 1.0) * 0.5 + 1e-9), bfb = b - bfa * (bfa + 1) / 2;     // b = fa(fa+1)/2 + fb
        P.wblk[g] = b | (bfa == bfb ? 256 : 0) | (items[q].part << 9) | (bfa << 13) | (bfb << 17) | ((items[q].np - 1) << 21);      // parts of a block sit in consecutive groups
        P.g_blk[g] = b; P.g_part[g] = items[q].part; P.g_np[g] = items[q].np;
    }
}

// second pass: the lists.  Every thread builds the lists of a contiguous range of chunks into its own vector (offsets relative to it); the ranges are
// concatenated in chunk order afterwards, so the result does not depend on the thread count
int write_lists(PackPlan& P, const ChunkEntries& chunk_entries, std::string& err) {
    DevWin& h = P.h; std::vector<int>& chunks = P.chunks; const int n_ch = P.n_chunks();
    const int *g_blk = P.g_blk, *g_part = P.g_part, *g_np = P.g_np;
    struct Part { std::vector<int> lists; int max_used = 0; bool overflow = false; int q0 = 0, q1 = 0; };
    std::vector<Part> part((size_t)std::max(P.threads, 1));
    const bool dbg_lists = std::getenv("UVS_DEBUG_LISTS") != nullptr;
    pack_parallel(n_ch, dbg_lists ? 1 : P.threads, [&](int q0, int q1, int t) {
        Part& T = part[t]; T.q0 = q0; T.q1 = q1;
        // A group's list is a contiguous slice [n p / np, n (p + 1) / np) of its block's entries in generation order; with the counts of the first pass the
        // destination of every entry is known before it is generated, so the entries go straight to their place (no per-block vectors: they were half of
        // the packing time of a canonical window).
        int first_grp[UVS_NBLKX2], blk_np[UVS_NBLKX2];
        for (int b = 0; b < UVS_NBLKX2; ++b) { first_grp[b] = -1; blk_np[b] = 0; }
        for (int g = 0; g < NG; ++g) if (g_blk[g] >= 0) { blk_np[g_blk[g]] = g_np[g]; if (g_part[g] == 0) first_grp[g_blk[g]] = g; }
        int dst[2][NG], lo_of[2][NG], fill[2][UVS_NBLKX2], cur_part[2][UVS_NBLKX2], cur_hi[2][UVS_NBLKX2];
        for (int qc = q0; qc < q1; ++qc) {
            const int* cS = P.cnt_s.data() + (size_t)qc * UVS_NBLKX2; const int* cD = P.cnt_d.data() + (size_t)qc * UVS_NBLKX2;
            chunks[UVS_CHUNK_INTS * qc + 3] = (int)T.lists.size();      // relative to this part for now
            const size_t base = T.lists.size();
            int at = 0;
            for (int pass = 0; pass < 2; ++pass) {
                const int* cnt = pass == 0 ? cS : cD;
                for (int g = 0; g < NG; ++g) {
                    dst[pass][g] = at; lo_of[pass][g] = 0;
                    if (g_blk[g] < 0) continue;
                    const long n = cnt[g_blk[g]], lo = n * g_part[g] / g_np[g], hi = n * (g_part[g] + 1) / g_np[g];
                    lo_of[pass][g] = (int)lo; at += (int)(hi - lo);
                }
            }
            const int n_ent = at;
            T.lists.resize(base + kListHdr + n_ent);
            int* hdrp = T.lists.data() + base; int* ent = hdrp + kListHdr;
            for (int pass = 0; pass < 2; ++pass) {
                for (int g = 0; g < NG; ++g) hdrp[pass * (NG + 1) + g] = dst[pass][g];
                hdrp[pass * (NG + 1) + NG] = pass == 0 ? dst[1][0] : n_ent;
            }
            // (the entries of a block arrive in order, so its current part and that part's end are carried along: no division per entry)
            for (int b = 0; b < UVS_NBLKX2; ++b) for (int pass = 0; pass < 2; ++pass) {
                fill[pass][b] = 0; cur_part[pass][b] = 0;
                const long n = (pass == 0 ? cS : cD)[b];
                cur_hi[pass][b] = blk_np[b] > 0 ? (int)(n / blk_np[b]) : 0;
                while (blk_np[b] > 0 && cur_part[pass][b] + 1 < blk_np[b] && cur_hi[pass][b] == 0) { ++cur_part[pass][b]; cur_hi[pass][b] = (int)(n * (cur_part[pass][b] + 1) / blk_np[b]); }      // leading empty parts
            }
            const auto put = [&](int pass, int b, int v) {
                const int np_ = blk_np[b];
                if (np_ <= 0) return;      // (a block without a group has no work by construction)
                const int e = fill[pass][b]++;
                while (e >= cur_hi[pass][b] && cur_part[pass][b] + 1 < np_) { ++cur_part[pass][b]; cur_hi[pass][b] = (int)((long)(pass == 0 ? cS : cD)[b] * (cur_part[pass][b] + 1) / np_); }
                const int g = first_grp[b] + cur_part[pass][b];
                ent[dst[pass][g] + (e - lo_of[pass][g])] = v;
            };
            chunk_entries(qc, [&](int b, int v) { put(0, b, v); }, [&](int b, int v) { put(1, b, v); });
            chunks[UVS_CHUNK_INTS * qc + 4] = (int)(T.lists.size() - base);
            {   // the chunk as the kernel lays it out must fit the staging area: records + Schur factors + the lists just built (an estimate that
                // is too small would let the lists run over the LM state that follows S in LDS)
                const int type = chunks[UVS_CHUNK_INTS * qc], nlm = chunks[UVS_CHUNK_INTS * qc + 2] - chunks[UVS_CHUNK_INTS * qc + 1], nob = chunks[UVS_CHUNK_INTS * qc + 7];
                const long used = chunk_doubles(h, type, nob, nlm, (long)(T.lists.size() - base));
                if (used > kStageCap) T.overflow = true;
                T.max_used = std::max(T.max_used, (int)used);
            }
            if (dbg_lists) {
                fprintf(stderr, "chunk %d type %d lm [%d,%d):\n", qc, chunks[UVS_CHUNK_INTS * qc], chunks[UVS_CHUNK_INTS * qc + 1], chunks[UVS_CHUNK_INTS * qc + 2]);
                for (int wv = 0; wv < NW; ++wv) {
                    fprintf(stderr, "  wave %d:", wv);
                    for (int q = 0; q < GPW; ++q) { const int g = wv * GPW + q; fprintf(stderr, " b%d.%d(%d,%d)", g_blk[g], g_part[g], T.lists[base + g + 1] - T.lists[base + g], T.lists[base + NG + 2 + g] - T.lists[base + NG + 1 + g]); }
                    fprintf(stderr, "\n");
                }
            }
        }
    });
    size_t total = 0;
    for (const auto& T : part) total += T.lists.size();
    P.lists.resize(total);
    size_t at = 0;
    for (const Part& T : part) {
        if (T.overflow) { err = "internal: chunk layout exceeds the LDS staging area"; return UVS_ERR_CAPACITY; }
        h.max_chunk_doubles = std::max(h.max_chunk_doubles, T.max_used);
        if (!T.lists.empty()) std::memcpy(P.lists.data() + at, T.lists.data(), T.lists.size() * sizeof(int));
        for (int qc = T.q0; qc < T.q1; ++qc) chunks[UVS_CHUNK_INTS * qc + 3] += (int)at;      // part-relative -> absolute (parts are in chunk order: thread t took the t-th range)
        at += T.lists.size();
    }
    return UVS_OK;
}

// what the kernels may assume of this window (chol_half_ok, redamp_ok) and what of S the prior touches (pblk, n_cimg)
void solver_flags(PackPlan& P) {
    DevWin& h = P.h; const uvs_window* w = P.w; const std::vector<int>& chunks = P.chunks;
    h.n_chunks = P.n_chunks();
    h.chol_half_ok = 1;
    if (P.have_prior) for (int b = 0; b < w->prior->n_blocks; ++b) if (w->prior->block_kind[b] == UVS_BLOCK_SPEEDBIAS && w->prior->block_frame[b] >= 2) h.chol_half_ok = 0;
    if (std::getenv("UVS_CHOL_FULL_ROWS")) h.chol_half_ok = 0;
    // re-damping (uvs_solve_kernel.h: redamp_chunk) keeps its per-line table and gradient rows in the record area of a line chunk
    h.redamp_ok = (!P.td_on && !P.ex_on && !P.relo_on) ? 1 : 0;
    for (int qc = 0; qc < h.n_chunks && h.redamp_ok; ++qc) {
        const long nob = chunks[UVS_CHUNK_INTS * qc + 7], nlm = chunks[UVS_CHUNK_INTS * qc + 2] - chunks[UVS_CHUNK_INTS * qc + 1];
        if (chunks[UVS_CHUNK_INTS * qc] == 1) { if (34 * nlm + 6 * nob > (long)UVS_LN_REC * nob) h.redamp_ok = 0; }
        // point chunk: redamp_chunk's gradient rows Gb[(nob + nlm)][6] sit in front of the E rows at rec + nob * pt_rec -- a chunk made mostly of landmarks WITHOUT observations would run into them
        else if (6 * (nob + nlm) > (long)h.pt_rec * nob) h.redamp_ok = 0;
    }
    if (!P.have_prior) return;
    const uvs_prior& p = *w->prior;
    // S blocks touched by the prior (all pairs of frames that own a kept pose / speed-bias block)
    bool in[UVS_NUM_FRAMES] = {false};
    for (int b = 0; b < p.n_blocks; ++b)
        if (p.block_kind[b] == UVS_BLOCK_POSE || p.block_kind[b] == UVS_BLOCK_SPEEDBIAS) in[p.block_frame[b]] = true;
        else if (p.block_kind[b] == UVS_BLOCK_TD && P.td_on) in[UVS_NUM_FRAMES - 1] = true;       // td lives in the last frame's block row
        else if (p.block_kind[b] == UVS_BLOCK_EX_POSE && P.ex_on) for (int q = 0; q < 6; ++q) in[q] = true;      // ex dofs live in frames 0..5
    for (int fa = 0; fa < UVS_NUM_FRAMES; ++fa) for (int fb = 0; fb <= fa; ++fb) if (in[fa] && in[fb]) P.pblk[P.n_pblk++] = (fa * (fa + 1) / 2 + fb) | (fa << 8) | (fb << 12);      // block | fa << 8 | fb << 12
    h.n_pblk = P.n_pblk;
    // compact image: only the entries whose row AND column are prior columns (a pose block owns 6 of the 16 rows of its S block, so 36 of 272
    // entries of a pose-pose block): what the per-linearization add reads (value + S offset) shrinks from 15 k to ~2.6 k entries
    // (the table itself is generated on the device: setup_window)
    bool mapped_s[UVS_RD] = {false}; int mapped = 0;
    for (int b = 0; b < p.n_blocks; ++b) for (int q = 0; q < prior_block_dofs(p, b); ++q) { const int si = prior_s_index(p, b, q, P.td_on, P.ex_on); if (si >= 0 && !mapped_s[si]) { mapped_s[si] = true; ++mapped; } }
    h.n_cimg = mapped * (mapped + 1) / 2;      // pairs of mapped S indices i >= j
}

// offsets of the blob's sections: doubles first (ONE prefix: a structure-cache hit sends only it), then the int tables; a pure function of the header's counts and options
void layout_blob(DevWin& h, size_t list_ints) {
    int d = (int)((sizeof(DevWin) + 7) / 8);
    h.d_frames = d; d += UVS_XDIM;
    h.d_invd = d; d += rup(std::max(h.n_points, 1), 2);
    h.d_ptmeas = d; d += 6 * h.pt_stride;
    h.d_ptvel = d; d += h.td_on ? 6 * h.pt_stride : 0;
    h.d_line = d; d += 4 * std::max(h.n_lines, 1);
    h.d_lnmeas = d; d += 9 * h.ln_stride;
    h.d_imu = d; d += std::max(h.n_imu, 1) * UVS_IMU_STRIDE;
    h.d_prior = d; d += h.prior_n * h.prior_n + 2 * h.prior_n + 144;
    int i = 2 * d;
    h.i_pt_lm = i; i += h.pt_stride; h.i_pt_fi = i; i += h.pt_stride; h.i_pt_fj = i; i += h.pt_stride; h.i_pt_beg = i; i += rup(h.n_points + 1, 2);
    h.i_pt_eidx = i; i += h.relo_on ? h.pt_stride : 0;
    h.i_ln_lm = i; i += h.ln_stride; h.i_ln_fj = i; i += h.ln_stride; h.i_ln_vp = i; i += h.ln_stride; h.i_ln_beg = i; i += rup(h.n_lines + 1, 2);
    h.i_imu = i; i += 2 * std::max(h.n_imu, 1);
    h.i_prior = i; i += 80 + UVS_MAX_PRIOR_DIM + UVS_RD + UVS_NBLK;
    h.i_chunks = i; i += UVS_CHUNK_INTS * std::max(h.n_chunks, 1);
    h.i_wblk = i; i += NG;
    h.i_lists = i; i += (int)list_ints + 2;
    h.blob_bytes = rup(4 * i, 256);
}

// offsets of the workspace's sections, likewise
void layout_workspace(DevWin& h) {
    const int XS = h.pt_xslots;
    int wsz = 0;
    h.w_invd0 = wsz; wsz += rup(std::max(h.n_points, 1), 2); h.w_invd1 = wsz; wsz += rup(std::max(h.n_points, 1), 2);
    h.w_line0 = wsz; wsz += 4 * std::max(h.n_lines, 1); h.w_line1 = wsz; wsz += 4 * std::max(h.n_lines, 1);
    h.w_ltrig0 = wsz; wsz += 8 * std::max(h.n_lines, 1); h.w_ltrig1 = wsz; wsz += 8 * std::max(h.n_lines, 1);
    h.w_scale_pt = wsz; wsz += rup(std::max(h.n_points, 1), 2); h.w_scale_ln = wsz; wsz += 4 * std::max(h.n_lines, 1);
    h.w_pt_E = wsz; wsz += 6 * (h.n_pt_obs + XS * h.n_points) + 6; h.w_pt_x = wsz; wsz += 4 * std::max(h.n_points, 1);
    h.w_ln_Y = wsz; wsz += 24 * std::max(h.n_ln_obs, 1); h.w_ln_x = wsz; wsz += UVS_LN_X * std::max(h.n_lines, 1);
    h.w_imu = wsz; wsz += std::max(h.n_imu, 1) * UVS_WIMU_STRIDE;
    h.w_imu_w = wsz; wsz += std::max(h.n_imu, 1) * UVS_IMU_WS;
    h.w_out = wsz; wsz += UVS_XDIM + std::max(h.n_points, 0) + 4 * std::max(h.n_lines, 0);
    h.w_prior_h0 = wsz; wsz += UVS_PH_DOUBLES(h.prior_n);      // H0 = J0^T J0, g0, c0, diag(H0) per S index: written once per solve by setup_window
    h.w_cimg = wsz; wsz += h.n_cimg + 2;      // 2 x n_cimg ints
    h.w_relo2 = wsz; if (h.relo2) wsz += UVS_RELO2_DOUBLES;
    h.w_gacc = wsz; wsz += 8 * UVS_GROWS * UVS_GT;      // (the 512-thread k_solve: gather accumulators of the last linearization)
    h.ws_doubles = rup(wsz, 32);
}

// the tables (index bookkeeping) of a zeroed blob B
void write_tables(const PackPlan& P, char* B) {
    const DevWin& h = P.h; const uvs_window* w = P.w;
    int* I = (int*)B;
    if (P.relo_on) for (int k = 0; k < h.n_pt_obs; ++k) I[h.i_pt_eidx + k] = P.eidx[k];
    for (int k = 0; k < h.n_pt_obs; ++k) { I[h.i_pt_lm + k] = w->pt_lm[k]; I[h.i_pt_fi + k] = w->pt_fi[k]; I[h.i_pt_fj + k] = w->pt_fj[k]; }
    for (int k = 0; k <= h.n_points; ++k) I[h.i_pt_beg + k] = P.pbeg[k];
    for (int k = 0; k < h.n_ln_obs; ++k) { I[h.i_ln_lm + k] = w->ln_lm[k]; I[h.i_ln_fj + k] = w->ln_fj[k]; I[h.i_ln_vp + k] = w->ln_has_vp[k] ? 1 : 0; }
    for (int k = 0; k <= h.n_lines; ++k) I[h.i_ln_beg + k] = P.lbeg[k];
    for (int b = 0; b < h.n_imu; ++b) { I[h.i_imu + 2 * b] = w->imu[b].frame_i; I[h.i_imu + 2 * b + 1] = w->imu[b].skip ? 1 : 0; }
    if (P.have_prior) {
        const uvs_prior& p = *w->prior;
        int* pt = I + h.i_prior;
        for (int q = 0; q < 80 + UVS_MAX_PRIOR_DIM + UVS_RD + UVS_NBLK; ++q) pt[q] = -1;
        for (int b = 0; b < p.n_blocks; ++b) {
            pt[b] = p.block_kind[b]; pt[16 + b] = p.block_frame[b]; pt[32 + b] = p.block_size[b]; pt[48 + b] = p.block_idx[b]; pt[64 + b] = p.x0_off[b];
            for (int q = 0; q < prior_block_dofs(p, b); ++q) {
                const int si = prior_s_index(p, b, q, P.td_on, P.ex_on);
                pt[80 + p.block_idx[b] + q] = si;
                if (si >= 0) pt[80 + UVS_MAX_PRIOR_DIM + si] = p.block_idx[b] + q;      // S index -> prior column
            }
        }
        for (int q = 0; q < P.n_pblk; ++q) pt[80 + UVS_MAX_PRIOR_DIM + UVS_RD + q] = P.pblk[q];
    }
    for (size_t q = 0; q < P.chunks.size(); ++q) I[h.i_chunks + q] = P.chunks[q];
    if (!P.lists.empty()) std::memcpy(I + h.i_lists, P.lists.data(), P.lists.size() * sizeof(int));
    for (int q = 0; q < NG; ++q) I[h.i_wblk + q] = P.wblk[q];
}

}  // namespace

int pack_window(const uvs_window* w_in, const uvs_options& opts, std::vector<char>& out, DevWin& hdr, std::string& err, int chunk_grid, PackCache* cache, PackDst* dst, bool all_blocks) {
    if (cache && cache->matches(w_in, opts, chunk_grid, all_blocks) && out.size() == (size_t)cache->hdr.blob_bytes) {      // same structure as the blob still sitting in `out`: values only
        fill_values(out.data(), cache->hdr, w_in, opts.estimate_td != 0, pack_inner_threads(w_in->n_point_obs + w_in->n_line_obs));
        hdr = cache->hdr;
        return UVS_OK;
    }
    if (cache) { cache->valid = false; cache->device_holds_tables = false; out.clear(); }
    const bool prof_ = std::getenv("UVS_PACK_PROFILE") != nullptr;
    auto t_prev_ = std::chrono::steady_clock::now();
    auto lap_ = [&](const char* what) { if (prof_) { const auto n_ = std::chrono::steady_clock::now(); fprintf(stderr, "pack %-10s %.3f ms\n", what, std::chrono::duration<double, std::milli>(n_ - t_prev_).count()); t_prev_ = n_; } };
    int rc = validate_window(w_in, err);
    if (rc != UVS_OK) return rc;
    lap_("validate");
    PackPlan P;
    P.w = w_in; P.td_on = opts.estimate_td != 0; P.ex_on = opts.estimate_extrinsic != 0; P.chunk_grid = chunk_grid; P.all_blocks = all_blocks;
    const int n_relo = w_in->n_relo_obs;
    if (n_relo < 0) { err = "bad counts"; return UVS_ERR_INVALID_ARG; }
    if (P.td_on && w_in->n_point_obs > 0 && (!w_in->pt_vel_i || !w_in->pt_vel_j || !w_in->pt_td_i || !w_in->pt_td_j)) { err = "estimate_td needs pt_vel_i / pt_vel_j / pt_td_i / pt_td_j"; return UVS_ERR_INVALID_ARG; }
    if (n_relo > 0 && (rc = merge_relocalization(w_in, P, err)) != UVS_OK) return rc;
    start_header(P, n_relo);
    DevWin& h = P.h;
    landmark_csr(P);
    if ((rc = split_chunks(P, err)) != UVS_OK) return rc;
    lap_("split");
    P.threads = pack_inner_threads(h.n_pt_obs + h.n_ln_obs);
    const ChunkEntries chunk_entries(P);
    count_entries(P, chunk_entries);
    lap_("entries");
    assign_groups(P);
    lap_("groups");
    if ((rc = write_lists(P, chunk_entries, err)) != UVS_OK) return rc;
    solver_flags(P);
    lap_("lists");
    layout_blob(h, P.lists.size());
    layout_workspace(h);
    char* B = nullptr;
    if (dst && dst->base) {      // straight into the pinned staging buffer when it has room (blob offsets are multiples of 256 bytes either way)
        const size_t at = dst->bump->fetch_add((size_t)h.blob_bytes);
        if (at + (size_t)h.blob_bytes <= dst->cap) { B = dst->base + at; dst->off = (long long)at; std::memset(B, 0, (size_t)h.blob_bytes); }
    }
    if (!B) {
        const size_t base = out.size();
        out.resize(base + h.blob_bytes, 0);
        B = out.data() + base;
    }
    fill_values(B, h, P.w, P.td_on, P.threads);
    write_tables(P, B);
    lap_("blob");
    hdr = h;
    if (cache && !P.relo_on && h.n_pt_obs + h.n_ln_obs >= kPackCacheMinObs) cache->store(w_in, opts, chunk_grid, all_blocks, h);
    return UVS_OK;
}

}  // namespace uvspack
