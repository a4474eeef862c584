// pose_graph.h -- mirror of the optimizer half of pose_graph/src/pose_graph.{h,cpp} and keyframe.{h,cpp} (loop closure): the keyframe list,
// the sequence shift and drift bookkeeping of addKeyFrame (:42-211), updateKeyFrameLoop (:888-...) / KeyFrame::updateLoop (keyframe.cpp:571-578)
// and a synchronous optimize4DoF (:403-579) whose ceres::Solve is uvs_pg_optimize().  Loop DETECTION (BRIEF, DBoW2, findConnection's PnP-RANSAC)
// is not mirrored: addKeyFrame takes the loop as the caller found it.  No polling thread, no save / load, no visualization.
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

    KeyFrame(double stamp, int seq, const Eigen::Vector3d& vio_T, const Eigen::Matrix3d& vio_R)
        : time_stamp(stamp), sequence(seq), vio_T_w_i(vio_T), T_w_i(vio_T), vio_R_w_i(vio_R), R_w_i(vio_R) {}
    void getVioPose(Eigen::Vector3d& P, Eigen::Matrix3d& R) const { P = vio_T_w_i; R = vio_R_w_i; }
    void getPose(Eigen::Vector3d& P, Eigen::Matrix3d& R) const { P = T_w_i; R = R_w_i; }
    void updatePose(const Eigen::Vector3d& P, const Eigen::Matrix3d& R) { T_w_i = P; R_w_i = R; }
    void updateVioPose(const Eigen::Vector3d& P, const Eigen::Matrix3d& R) { vio_T_w_i = P; vio_R_w_i = R; T_w_i = P; R_w_i = R; }
    Eigen::Vector3d getLoopRelativeT() const { return Eigen::Vector3d(loop_info[0], loop_info[1], loop_info[2]); }
    Eigen::Quaterniond getLoopRelativeQ() const { return Eigen::Quaterniond(loop_info[3], loop_info[4], loop_info[5], loop_info[6]); }
    double getLoopRelativeYaw() const { return loop_info[7]; }
    void updateLoop(const LoopInfo& info);
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

  private:
    uvs_pose_graph* pg_ = nullptr;
};
