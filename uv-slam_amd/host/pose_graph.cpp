// pose_graph.cpp -- see pose_graph.h.  Reference line numbers are those of pose_graph/src/pose_graph.cpp.
#include "pose_graph.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include "utility.h"

void KeyFrame::updateLoop(const LoopInfo& info) {          // keyframe.cpp:571-578
    if (std::fabs(info[7]) < 30.0 && std::sqrt(info[0] * info[0] + info[1] * info[1] + info[2] * info[2]) < 20.0) loop_info = info;
}

KeyFrame::KeyFrame(double stamp, int index_, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R, const uint8_t* image, int width, int height,
                   const std::vector<Eigen::Vector3d>& point_3d_, const std::vector<std::array<float, 2>>& point_2d_uv_,
                   const std::vector<std::array<double, 2>>& point_2d_norm_, const std::vector<double>& point_id_, int sequence_,
                   uvs_kf_extractor* extractor, const uvs_kf_camera& camera)
    : KeyFrame(stamp, sequence_, vio_T, vio_R) {             // keyframe.cpp:14-41
    index = index_;
    point_3d = point_3d_; point_2d_uv = point_2d_uv_; point_2d_norm = point_2d_norm_; point_id = point_id_;
    (void)uvs_kf_set_camera_model(extractor, nullptr);      // a model an earlier keyframe left on the extractor would lift this one's keypoints
    extractOnline(image, width, height, extractor, &camera);
}

KeyFrame::KeyFrame(double stamp, int index_, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R, const uint8_t* image, int width, int height,
                   const std::vector<Eigen::Vector3d>& point_3d_, const std::vector<std::array<float, 2>>& point_2d_uv_,
                   const std::vector<std::array<double, 2>>& point_2d_norm_, const std::vector<double>& point_id_, int sequence_,
                   uvs_kf_extractor* extractor, const uvs_camera_model& model)
    : KeyFrame(stamp, sequence_, vio_T, vio_R) {
    index = index_;
    point_3d = point_3d_; point_2d_uv = point_2d_uv_; point_2d_norm = point_2d_norm_; point_id = point_id_;
    const int rc = uvs_kf_set_camera_model(extractor, &model);
    if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_kf_set_camera_model: ") + uvs_status_string(rc) + " / " + uvs_kf_last_error(extractor));
    extractOnline(image, width, height, extractor, nullptr);
}

void KeyFrame::extractOnline(const uint8_t* image, int width, int height, uvs_kf_extractor* extractor, const uvs_kf_camera* camera) {
    uvs_kf_frame fr;
    fr.image = image; fr.width = width; fr.height = height; fr.n_window = (int)point_2d_uv.size(); fr.reserved = 0;
    fr.window_uv = point_2d_uv.empty() ? nullptr : point_2d_uv[0].data();
    // one frame: the strided keypoint arrays start at 0, and no handle returns more than UVS_LC_MAX_OLD keypoints
    std::vector<std::array<int32_t, 2>> xy(UVS_LC_MAX_OLD);
    std::vector<uint8_t> score(UVS_LC_MAX_OLD);
    std::vector<std::array<double, 2>> norm(UVS_LC_MAX_OLD);
    std::vector<std::array<uint64_t, 4>> desc(UVS_LC_MAX_OLD);
    window_brief_descriptors.resize(std::max<size_t>(point_2d_uv.size(), 1));
    const int rc = uvs_kf_extract(extractor, 1, &fr, camera, xy[0].data(), score.data(), norm[0].data(), desc[0].data(),
                                  window_brief_descriptors[0].data(), &last_extract);
    if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_kf_extract: ") + uvs_status_string(rc) + " / " + uvs_kf_last_error(extractor));
    window_brief_descriptors.resize(point_2d_uv.size());
    const size_t n = (size_t)last_extract.n_returned;
    keypoints.assign(xy.begin(), xy.begin() + n);
    keypoints_norm.assign(norm.begin(), norm.begin() + n);
    brief_descriptors.assign(desc.begin(), desc.begin() + n);
}

bool KeyFrame::findConnection(KeyFrame* old_kf, uvs_loop_verifier* lc, const Eigen::Vector3d& tic, const Eigen::Quaterniond& qic) {
    const int n = (int)point_3d.size();
    std::vector<double> p3d(3 * (size_t)n);
    for (int i = 0; i < n; ++i) { p3d[3 * i] = point_3d[i].x(); p3d[3 * i + 1] = point_3d[i].y(); p3d[3 * i + 2] = point_3d[i].z(); }
    const Eigen::Quaterniond q = Eigen::Quaterniond(origin_vio_R).normalized();
    uvs_lc_pair p;
    p.n_query = n; p.n_old = (int)old_kf->keypoints_norm.size();
    p.p3d = p3d.data(); p.desc = window_brief_descriptors.empty() ? nullptr : window_brief_descriptors[0].data();
    p.vio_t[0] = origin_vio_T.x(); p.vio_t[1] = origin_vio_T.y(); p.vio_t[2] = origin_vio_T.z();
    p.vio_q[0] = q.x(); p.vio_q[1] = q.y(); p.vio_q[2] = q.z(); p.vio_q[3] = q.w();
    p.old_uv_norm = old_kf->keypoints_norm.empty() ? nullptr : old_kf->keypoints_norm[0].data();
    p.old_desc = old_kf->brief_descriptors.empty() ? nullptr : old_kf->brief_descriptors[0].data();
    p.seed = ((uint64_t)(uint32_t)index << 32) | (uint64_t)(uint32_t)old_kf->index;
    const double t[3] = {tic.x(), tic.y(), tic.z()}, qx[4] = {qic.x(), qic.y(), qic.z(), qic.w()};
    std::vector<int32_t> match_old(std::max(n, 1));
    std::vector<uint8_t> inlier(std::max(n, 1));
    if ((int)window_brief_descriptors.size() != n || old_kf->brief_descriptors.size() != old_kf->keypoints_norm.size() ||
        uvs_lc_verify(lc, 1, &p, t, qx, match_old.data(), inlier.data(), &last_verify) != UVS_OK) {
        last_verify = uvs_lc_result{}; last_verify.reason = -1;
        return false;
    }
    matched_2d_old_norm.clear(); matched_id.clear();                 // :392-399, the PnP inliers in query order
    for (int i = 0; i < n; ++i)
        if (inlier[i]) {
            matched_2d_old_norm.push_back(old_kf->keypoints_norm[match_old[i]]);
            matched_id.push_back(i < (int)point_id.size() ? point_id[i] : (double)i);
        }
    if (!last_verify.accepted) return false;
    has_loop = true; loop_index = old_kf->index;                     // :478-487
    for (int k = 0; k < 8; ++k) loop_info[k] = last_verify.loop_info[k];
    return true;
}

PoseGraph::PoseGraph(int device, int max_keyframes, int max_loops) : device_(device) {
    sequence_loop.push_back(0);                             // :14
    int rc = uvs_pg_create(device, max_keyframes, max_loops, &pg_);
    if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_pg_create: ") + uvs_status_string(rc));
    rc = uvs_lc_create(device, 1, UVS_LC_MAX_QUERY, UVS_LC_MAX_OLD, &lc_);
    if (rc != UVS_OK) { uvs_pg_destroy(pg_); throw std::runtime_error(std::string("uvs_lc_create: ") + uvs_status_string(rc)); }
}

PoseGraph::~PoseGraph() {
    uvs_pg_destroy(pg_);
    uvs_lc_destroy(lc_);
    uvs_pr_destroy(pr_);
    for (KeyFrame* kf : keyframelist) delete kf;
}

void PoseGraph::loadVocabulary(int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t* node_id, const int32_t* parent_id,
                               const double* weight, const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id,
                               int max_features, int initial_entries) {
    uvs_place_recognizer* pr = nullptr;
    char msg[256] = "";
    int rc = uvs_pr_check_vocabulary(k, L, scoring_type, weighting_type, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_node_id, word_id,
                                     msg, (int)sizeof msg);
    if (rc == UVS_OK)
        rc = uvs_pr_create(device_, k, L, scoring_type, weighting_type, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_node_id, word_id,
                           max_features, initial_entries, &pr);
    if (rc != UVS_OK) throw std::runtime_error(std::string("loadVocabulary: ") + uvs_status_string(rc) + " / " + msg);
    uvs_pr_destroy(pr_);
    pr_ = pr;
}

void PoseGraph::loadVocabulary(const std::string& path) {      // ThirdParty/VocabularyBinary.cpp:27-35 deserialize
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("loadVocabulary: cannot open " + path);
    int32_t head[6];                                           // k, L, scoringType, weightingType, nNodes, nWords
    bool ok = std::fread(head, sizeof head, 1, f) == 1 && head[4] >= 0 && head[5] >= 0;
    std::vector<char> nodes, words;
    if (ok) {
        nodes.resize((size_t)head[4] * 48); words.resize((size_t)head[5] * 8);
        ok = (nodes.empty() || std::fread(nodes.data(), nodes.size(), 1, f) == 1) && (words.empty() || std::fread(words.data(), words.size(), 1, f) == 1);
    }
    std::fclose(f);
    if (!ok) throw std::runtime_error("loadVocabulary: " + path + " is shorter than its header says");
    const size_t nn = (size_t)head[4], nw = (size_t)head[5];
    std::vector<int32_t> node_id(nn), parent_id(nn), word_node_id(nw), word_id(nw);
    std::vector<double> weight(nn);
    std::vector<uint64_t> descriptor(4 * nn);
    for (size_t i = 0; i < nn; ++i) {                          // {int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]}
        const char* r = nodes.data() + 48 * i;
        std::memcpy(&node_id[i], r, 4); std::memcpy(&parent_id[i], r + 4, 4); std::memcpy(&weight[i], r + 8, 8); std::memcpy(&descriptor[4 * i], r + 16, 32);
    }
    for (size_t i = 0; i < nw; ++i) {                          // {int32 nodeId, int32 wordId}
        std::memcpy(&word_node_id[i], words.data() + 8 * i, 4); std::memcpy(&word_id[i], words.data() + 8 * i + 4, 4);
    }
    loadVocabulary(head[0], head[1], head[2], head[3], head[4], node_id.data(), parent_id.data(), weight.data(), descriptor.data(), head[5],
                   word_node_id.data(), word_id.data());
}

int PoseGraph::detectLoop(KeyFrame* keyframe, int frame_index) {
    last_detect_ids.assign(UVS_PR_DETECT_RESULTS, -1); last_detect_scores.assign(UVS_PR_DETECT_RESULTS, 0.0);
    if (!pr_) { last_error = "detectLoop: no vocabulary (loadVocabulary)"; last_detect_ids.clear(); last_detect_scores.clear(); return -1; }
    int32_t loop_index = -1, n_results = 0;
    const int n = (int)keyframe->brief_descriptors.size();
    const int rc = uvs_pr_detect(pr_, n, n ? keyframe->brief_descriptors[0].data() : nullptr, frame_index, &loop_index, &n_results,
                                 last_detect_ids.data(), last_detect_scores.data());
    if (rc != UVS_OK) { last_error = std::string("detectLoop: ") + uvs_pr_last_error(pr_); n_results = 0; loop_index = -1; }
    last_detect_ids.resize(n_results); last_detect_scores.resize(n_results);
    return loop_index;
}

void PoseGraph::addKeyFrameIntoVoc(KeyFrame* keyframe) {
    if (!pr_) { last_error = "addKeyFrameIntoVoc: no vocabulary (loadVocabulary)"; return; }
    const int32_t n = (int32_t)keyframe->brief_descriptors.size();
    int32_t id = -1;
    if (uvs_pr_add(pr_, 1, &n, n ? keyframe->brief_descriptors[0].data() : nullptr, &id) != UVS_OK)
        last_error = std::string("addKeyFrameIntoVoc: ") + uvs_pr_last_error(pr_);
}

bool PoseGraph::addKeyFrameDetectLoop(KeyFrame* cur_kf, bool flag_detect_loop) {
    int candidate = -1;                                        // :64-73; the index addKeyFrameImpl is about to give cur_kf is global_index
    if (flag_detect_loop) candidate = detectLoop(cur_kf, global_index);
    else addKeyFrameIntoVoc(cur_kf);
    last_candidate = candidate;
    addKeyFrameImpl(cur_kf, candidate, -1, nullptr);
    return cur_kf->has_loop;
}

KeyFrame* PoseGraph::getKeyFrame(int index) {
    for (KeyFrame* kf : keyframelist) if (kf->index == index) return kf;
    return nullptr;
}

void PoseGraph::addKeyFrame(KeyFrame* cur_kf, int loop_index, const LoopInfo* loop_info) {
    addKeyFrameImpl(cur_kf, -1, loop_index, loop_info);
}

bool PoseGraph::addKeyFrameWithCandidate(KeyFrame* cur_kf, int candidate_index) {
    addKeyFrameImpl(cur_kf, candidate_index, -1, nullptr);
    return cur_kf->has_loop;
}

void PoseGraph::addKeyFrameImpl(KeyFrame* cur_kf, int candidate_index, int loop_index, const LoopInfo* loop_info) {
    Eigen::Vector3d vio_P_cur;
    Eigen::Matrix3d vio_R_cur;
    if (sequence_cnt != cur_kf->sequence) {                 // :45-56 a new sequence starts in its own VIO frame
        sequence_cnt++;
        sequence_loop.push_back(0);
        w_t_vio = Eigen::Vector3d(0, 0, 0); w_r_vio = Eigen::Matrix3d::Identity();
        t_drift = Eigen::Vector3d(0, 0, 0); r_drift = Eigen::Matrix3d::Identity();
    }
    cur_kf->getVioPose(vio_P_cur, vio_R_cur);               // :58-62 shift to the base frame
    vio_P_cur = w_r_vio * vio_P_cur + w_t_vio;
    vio_R_cur = w_r_vio * vio_R_cur;
    cur_kf->updateVioPose(vio_P_cur, vio_R_cur);
    cur_kf->index = global_index++;
    if (candidate_index >= 0) {                             // :64-77 detectLoop's candidate, then findConnection
        KeyFrame* cand = getKeyFrame(candidate_index);
        if (cand && cur_kf->findConnection(cand, lc_, tic_, qic_)) { loop_index = candidate_index; loop_info = &cur_kf->loop_info; }
    }
    KeyFrame* old_kf = loop_index >= 0 ? getKeyFrame(loop_index) : nullptr;
    if (old_kf && loop_info) {                               // :75-121, with findConnection's outcome given
        cur_kf->has_loop = true; cur_kf->loop_index = loop_index; cur_kf->loop_info = *loop_info;
        if (earliest_loop_index > loop_index || earliest_loop_index == -1) earliest_loop_index = loop_index;
        Eigen::Vector3d w_P_old, w_P_cur;
        Eigen::Matrix3d w_R_old, w_R_cur;
        old_kf->getVioPose(w_P_old, w_R_old);
        cur_kf->getVioPose(vio_P_cur, vio_R_cur);
        const Eigen::Vector3d relative_t = cur_kf->getLoopRelativeT();
        const Eigen::Matrix3d relative_q = cur_kf->getLoopRelativeQ().toRotationMatrix();
        w_P_cur = w_R_old * relative_t + w_P_old;
        w_R_cur = w_R_old * relative_q;
        const double shift_yaw = Utility::R2ypr(w_R_cur).x() - Utility::R2ypr(vio_R_cur).x();
        const Eigen::Matrix3d shift_r = Utility::ypr2R(Eigen::Vector3d(shift_yaw, 0, 0));
        const Eigen::Vector3d shift_t = w_P_cur - w_R_cur * vio_R_cur.transpose() * vio_P_cur;
        if (old_kf->sequence != cur_kf->sequence && sequence_loop[cur_kf->sequence] == 0) {     // shift the whole new sequence
            w_r_vio = shift_r; w_t_vio = shift_t;
            vio_P_cur = w_r_vio * vio_P_cur + w_t_vio;
            vio_R_cur = w_r_vio * vio_R_cur;
            cur_kf->updateVioPose(vio_P_cur, vio_R_cur);
            for (KeyFrame* kf : keyframelist)
                if (kf->sequence == cur_kf->sequence) {
                    Eigen::Vector3d P; Eigen::Matrix3d R;
                    kf->getVioPose(P, R);
                    kf->updateVioPose(w_r_vio * P + w_t_vio, w_r_vio * R);
                }
            sequence_loop[cur_kf->sequence] = 1;
        }
    }
    Eigen::Vector3d P; Eigen::Matrix3d R;                    // :124-129 the current drift correction
    cur_kf->getVioPose(P, R);
    cur_kf->updatePose(r_drift * P + t_drift, r_drift * R);
    keyframelist.push_back(cur_kf);
}

void PoseGraph::updateKeyFrameLoop(int index, const LoopInfo& loop_info) {      // :888-892 (the FAST_RELOCALIZATION branch is not mirrored)
    if (KeyFrame* kf = getKeyFrame(index)) kf->updateLoop(loop_info);
}

int PoseGraph::optimize4DoF(int cur_index) {
    const int first_looped_index = earliest_loop_index;
    KeyFrame* cur_kf = getKeyFrame(cur_index);
    if (!cur_kf || first_looped_index < 0) { last_error = "optimize4DoF: no such keyframe or no loop yet"; return UVS_ERR_INVALID_ARG; }
    std::vector<double> t, q, euler;
    std::vector<int32_t> seq, constant;
    std::vector<uvs_pg_loop> loops;
    std::vector<KeyFrame*> kfs;
    int i = 0;
    for (KeyFrame* kf : keyframelist) {                      // :453-531
        if (kf->index < first_looped_index) continue;
        kf->local_index = i;
        Eigen::Vector3d tmp_t; Eigen::Matrix3d tmp_r;
        kf->getVioPose(tmp_t, tmp_r);
        const Eigen::Quaterniond tmp_q(tmp_r);
        t.insert(t.end(), {tmp_t.x(), tmp_t.y(), tmp_t.z()});
        q.insert(q.end(), {tmp_q.x(), tmp_q.y(), tmp_q.z(), tmp_q.w()});
        const Eigen::Vector3d e = Utility::R2ypr(tmp_q.toRotationMatrix());
        euler.insert(euler.end(), {e.x(), e.y(), e.z()});
        seq.push_back(kf->sequence);
        constant.push_back(kf->index == first_looped_index || kf->sequence == 0);
        if (kf->has_loop) {
            KeyFrame* old_kf = getKeyFrame(kf->loop_index);
            if (!old_kf || old_kf->index < first_looped_index) { last_error = "optimize4DoF: loop before first_looped_index"; return UVS_ERR_INVALID_ARG; }
            uvs_pg_loop l;
            l.cur = i; l.old = old_kf->local_index;
            const Eigen::Vector3d rt = kf->getLoopRelativeT();
            l.rel_t[0] = rt.x(); l.rel_t[1] = rt.y(); l.rel_t[2] = rt.z(); l.rel_yaw = kf->getLoopRelativeYaw();
            loops.push_back(l);
        }
        kfs.push_back(kf);
        if (kf->index == cur_index) break;
        i++;
    }
    uvs_pg_problem p;
    p.n = (int)kfs.size(); p.n_loops = (int)loops.size();
    p.t = t.data(); p.q = q.data(); p.sequence = seq.data(); p.constant = constant.data(); p.loops = loops.data();
    std::vector<double> yaw_t(4 * kfs.size());
    const int rc = uvs_pg_optimize(pg_, &p, yaw_t.data(), &last_report);
    if (rc != UVS_OK) { last_error = uvs_pg_last_error(pg_); return rc; }
    for (size_t k = 0; k < kfs.size(); ++k)                   // :555-568 write back ypr2R(yaw, pitch, roll), t
        kfs[k]->updatePose(Eigen::Vector3d(yaw_t[4 * k + 1], yaw_t[4 * k + 2], yaw_t[4 * k + 3]),
                           Eigen::Quaterniond(Utility::ypr2R(Eigen::Vector3d(yaw_t[4 * k], euler[3 * k + 1], euler[3 * k + 2]))).toRotationMatrix());
    Eigen::Vector3d cur_t, vio_t; Eigen::Matrix3d cur_r, vio_r;                // :570-577 drift
    cur_kf->getPose(cur_t, cur_r);
    cur_kf->getVioPose(vio_t, vio_r);
    yaw_drift = Utility::R2ypr(cur_r).x() - Utility::R2ypr(vio_r).x();
    r_drift = Utility::ypr2R(Eigen::Vector3d(yaw_drift, 0, 0));
    t_drift = cur_t - r_drift * vio_t;
    bool after = false;                                       // :582-591 every keyframe after cur
    for (KeyFrame* kf : keyframelist) {
        if (after) {
            Eigen::Vector3d P; Eigen::Matrix3d R;
            kf->getVioPose(P, R);
            kf->updatePose(r_drift * P + t_drift, r_drift * R);
        }
        if (kf == cur_kf) after = true;
    }
    return UVS_OK;
}

bool PoseGraph::writeTum(const std::string& path) const {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (const KeyFrame* kf : keyframelist) {
        const Eigen::Quaterniond Q(kf->R_w_i);
        std::fprintf(f, "%.9f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n", kf->time_stamp, kf->T_w_i.x(), kf->T_w_i.y(), kf->T_w_i.z(), Q.x(), Q.y(), Q.z(), Q.w());
    }
    return std::fclose(f) == 0;
}
