// pose_graph.h -- mirror of the optimizer half of pose_graph/src/pose_graph.{h,cpp} and keyframe.{h,cpp} (loop closure): the keyframe list,
// the sequence shift and drift bookkeeping of addKeyFrame (:42-211), updateKeyFrameLoop (:888-...) / KeyFrame::updateLoop (keyframe.cpp:571-578)
// and a synchronous optimize4DoF (:403-579) whose ceres::Solve is uvs_pg_optimize(); KeyFrame::findConnection (keyframe.cpp:259-521: BRIEF
// matching, PnP-RANSAC, the loop_info gates) runs on the GPU through uvs_lc_verify(), and the online KeyFrame constructor (keyframe.cpp:14-41:
// computeWindowBRIEFPoint, computeBRIEFPoint) extracts FAST corners, BRIEF descriptors and normalized keypoints from the image on the GPU
// through uvs_kf_extract().  Place recognition (detectLoop, :304-386, and addKeyFrameIntoVoc, :388-401: DBoW2's vocabulary tree, database and
// L1 query) runs on the GPU through uvs_pr_detect() / uvs_pr_add() once loadVocabulary() has been given the caller's vocabulary:
// addKeyFrameDetectLoop is the reference's addKeyFrame(cur_kf, flag_detect_loop).  addKeyFrameWithCandidate still takes the candidate from
// the caller, and addKeyFrame a loop as the caller found it.  A keyframe may also carry descriptors and normalized keypoints
// as the caller extracted them (the first constructor).  No thumbnail, no polling thread, no save / load, no visualization.
#pragma once
#include <array>
#include <list>
#include <string>
#include <vector>
#include "eigen_lite.h"
#include "../../include/uvs_solver.h"

// loop_info as in the reference (keyframe.cpp:485): relative t (3), relative q (w, x, y, z), relative yaw (deg)
typedef std::array<double, 8> LoopInfo;

struct KeyFrame {
    double time_stamp = 0.0;
    int index = -1, local_index = -1, sequence = 1;
    Eigen::Vector3d vio_T_w_i, T_w_i;
    Eigen::Matrix3d vio_R_w_i = Eigen::Matrix3d::Identity(), R_w_i = Eigen::Matrix3d::Identity();
    bool has_loop = false;
    int loop_index = -1;
    LoopInfo loop_info{};
    // what findConnection reads (keyframe.h): the VIO pose at creation (never shifted), the window points with their 3-D positions in that
    // VIO frame, their normalized coordinates, ids and BRIEF descriptors, and the keyframe's own keypoints (as an old keyframe)
    Eigen::Vector3d origin_vio_T;
    Eigen::Matrix3d origin_vio_R = Eigen::Matrix3d::Identity();
    std::vector<Eigen::Vector3d> point_3d;
    std::vector<std::array<float, 2>> point_2d_uv;         // cv::Point2f pixels (the online constructor's)
    std::vector<std::array<double, 2>> point_2d_norm;
    std::vector<double> point_id;
    std::vector<std::array<uint64_t, 4>> window_brief_descriptors;
    std::vector<std::array<double, 2>> keypoints_norm;
    std::vector<std::array<uint64_t, 4>> brief_descriptors;
    std::vector<std::array<int32_t, 2>> keypoints;         // FAST corners (x, y) in row-major order (the online constructor's)
    uvs_kf_result last_extract{};                          // counts and status of the online constructor's uvs_kf_extract
    // findConnection's inlier matches (matched_2d_old_norm, matched_id: what Estimator::setReloFrame takes) and its verdict
    std::vector<std::array<double, 2>> matched_2d_old_norm;
    std::vector<double> matched_id;
    uvs_lc_result last_verify{};

    KeyFrame(double stamp, int seq, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R)
        : time_stamp(stamp), sequence(seq), vio_T_w_i(vio_T), T_w_i(vio_T), vio_R_w_i(vio_R), R_w_i(vio_R), origin_vio_T(vio_T), origin_vio_R(vio_R) {}
    // "create keyframe online" (keyframe.cpp:14-41): window_brief_descriptors at point_2d_uv (computeWindowBRIEFPoint, :75-85), then keypoints,
    // brief_descriptors and keypoints_norm of the image's FAST corners (computeBRIEFPoint, :87-113), in one uvs_kf_extract call.  `image` is
    // width x height grey levels and is not kept.  On UVS_KF_OVERFLOW the keyframe carries the extractor's first max_keypoints corners
    // (last_extract.status tells).  Throws std::runtime_error when the call fails.
    KeyFrame(double stamp, int index_, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R, const uint8_t* image, int width, int height,
             const std::vector<Eigen::Vector3d>& point_3d_, const std::vector<std::array<float, 2>>& point_2d_uv_,
             const std::vector<std::array<double, 2>>& point_2d_norm_, const std::vector<double>& point_id_, int sequence_,
             uvs_kf_extractor* extractor, const uvs_kf_camera& camera);
    // the same for any camera model (a fisheye: MEI, Kannala-Brandt): the model is put on the extractor (uvs_kf_set_camera_model; a model the
    // extractor already holds is not uploaded again) and keypoints_norm are lifted through it.  The constructor above takes it off again
    KeyFrame(double stamp, int index_, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R, const uint8_t* image, int width, int height,
             const std::vector<Eigen::Vector3d>& point_3d_, const std::vector<std::array<float, 2>>& point_2d_uv_,
             const std::vector<std::array<double, 2>>& point_2d_norm_, const std::vector<double>& point_id_, int sequence_,
             uvs_kf_extractor* extractor, const uvs_camera_model& model);
    void getVioPose(Eigen::Vector3d& P, Eigen::Matrix3d& R) const { P = vio_T_w_i; R = vio_R_w_i; }
    // the body of the two online constructors; camera == nullptr: the extractor holds a camera model
    void extractOnline(const uint8_t* image, int width, int height, uvs_kf_extractor* extractor, const uvs_kf_camera* camera);
    void getPose(Eigen::Vector3d& P, Eigen::Matrix3d& R) const { P = T_w_i; R = R_w_i; }
    void updatePose(const Eigen::Vector3d& P, const Eigen::Matrix3d& R) { T_w_i = P; R_w_i = R; }
    void updateVioPose(const Eigen::Vector3d& P, const Eigen::Matrix3d& R) { vio_T_w_i = P; vio_R_w_i = R; T_w_i = P; R_w_i = R; }
    Eigen::Vector3d getLoopRelativeT() const { return Eigen::Vector3d(loop_info[0], loop_info[1], loop_info[2]); }
    Eigen::Quaterniond getLoopRelativeQ() const { return Eigen::Quaterniond(loop_info[3], loop_info[4], loop_info[5], loop_info[6]); }
    double getLoopRelativeYaw() const { return loop_info[7]; }
    void updateLoop(const LoopInfo& info);
    // keyframe.cpp:259-521 through uvs_lc_verify (one pair); true: has_loop, loop_index and loop_info are set.  The RANSAC seed is
    // (index << 32) | old_kf->index.  Returns false also when the call fails (the status is left in last_verify.reason = -1).
    bool findConnection(KeyFrame* old_kf, uvs_loop_verifier* lc, const Eigen::Vector3d& tic, const Eigen::Quaterniond& qic);
};

class PoseGraph {
  public:
    // device / capacities of the uvs_pose_graph handle (uvs_pg_create); throws std::runtime_error without a GPU (no CPU path)
    PoseGraph(int device = 0, int max_keyframes = 16384, int max_loops = 256);
    ~PoseGraph();
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;

    // takes ownership of cur_kf; loop_index = -1: no loop, else the loop (old keyframe, loop_info) as findConnection would have accepted it
    void addKeyFrame(KeyFrame* cur_kf, int loop_index = -1, const LoopInfo* loop_info = nullptr);
    void updateKeyFrameLoop(int index, const LoopInfo& loop_info);
    // addKeyFrame of the reference with place recognition's answer given: candidate_index = what detectLoop returned (-1: none).  The
    // sequence shift first, then cur_kf->findConnection(candidate) on the GPU, then addKeyFrame's loop bookkeeping (:75-121) when it passes.
    // Returns whether a loop was accepted.  Needs setExtrinsic() first.
    bool addKeyFrameWithCandidate(KeyFrame* cur_kf, int candidate_index);
    void setExtrinsic(const Eigen::Vector3d& tic, const Eigen::Quaterniond& qic) { tic_ = tic; qic_ = qic; }
    // the vocabulary of place recognition, as the arrays of the reference's binary file (ThirdParty/VocabularyBinary.hpp; the arguments of
    // uvs_pr_create) or as that file (the reference's support_files/brief_k10L6.bin).  Replaces an earlier vocabulary and empties the
    // database.  Throws std::runtime_error when the file cannot be read or uvs_pr_create fails.
    void loadVocabulary(int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t* node_id, const int32_t* parent_id,
                        const double* weight, const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id,
                        int max_features = UVS_LC_MAX_OLD, int initial_entries = 1024);
    void loadVocabulary(const std::string& path);
    // :304-386 through uvs_pr_detect: the query of the keyframe's brief_descriptors, their add, the score gates; -1: no candidate (also when
    // the call fails: last_error tells).  last_detect_ids / last_detect_scores keep the query's results.  Needs loadVocabulary() first.
    int detectLoop(KeyFrame* keyframe, int frame_index);
    // :388-401 through uvs_pr_add
    void addKeyFrameIntoVoc(KeyFrame* keyframe);
    // addKeyFrame(cur_kf, flag_detect_loop) of the reference (:42-211): detectLoop(cur_kf, its index) when the flag is set, and its answer
    // through addKeyFrameWithCandidate's path; otherwise addKeyFrameIntoVoc and addKeyFrame without a loop.  Returns whether a loop was accepted.
    bool addKeyFrameDetectLoop(KeyFrame* cur_kf, bool flag_detect_loop);
    // one pass of the reference's optimize4DoF loop body for cur_index (first_looped_index = earliest_loop_index); returns the uvs status
    int optimize4DoF(int cur_index);
    KeyFrame* getKeyFrame(int index);
    // the corrected path (T_w_i, R_w_i of every keyframe) as a result file: `stamp x y z qx qy qz qw` (trajectory.py's TUM layout)
    bool writeTum(const std::string& path) const;

    std::list<KeyFrame*> keyframelist;
    int earliest_loop_index = -1, global_index = 0, sequence_cnt = 0;
    std::vector<int> sequence_loop;
    Eigen::Vector3d t_drift, w_t_vio;
    Eigen::Matrix3d r_drift = Eigen::Matrix3d::Identity(), w_r_vio = Eigen::Matrix3d::Identity();
    double yaw_drift = 0.0;
    uvs_pg_report last_report{};
    std::string last_error;
    int last_candidate = -1;                               // what addKeyFrameDetectLoop's detectLoop returned
    std::vector<int32_t> last_detect_ids;
    std::vector<double> last_detect_scores;

  private:
    void addKeyFrameImpl(KeyFrame* cur_kf, int candidate_index, int loop_index, const LoopInfo* loop_info);
    uvs_pose_graph* pg_ = nullptr;
    uvs_loop_verifier* lc_ = nullptr;
    uvs_place_recognizer* pr_ = nullptr;
    int device_ = 0;
    Eigen::Vector3d tic_;
    Eigen::Quaterniond qic_;
};
