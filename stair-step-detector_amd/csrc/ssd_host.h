/*
 * ssd_host.h — what the two halves of the C ABI share: ssd_host.cpp (plain C++: every entry point that needs no handle, no stream and
 * no HIP call) defines these, ssd_capi.hip (the handle and everything that runs on it) uses them.  Internal to libssd_hip.so: hidden,
 * so the library exports what include/ssd_hip.h declares and nothing of this.  Nothing else belongs here.
 */
#ifndef SSD_HOST_H_
#define SSD_HOST_H_

#include "../../include/ssd_hip.h"
#include "ssd_ground.h"
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

/* the refusal every entry point of either file returns through: `msg` is what ssd_last_error() gives the calling thread from then on */
int fail(int code, const std::string &msg);

/* rs2::pointcloud's maps for a W x H image: W values of x, then H of y (ssd_set_intrinsics uploads what ssd_deproject_host uses) */
void depth_maps(const ssd_intrinsics &in, int W, int H, std::vector<float> &maps);

bool good_intrinsics(const ssd_intrinsics &in);
void ground_prior_fill(ssd::GroundPrior &g, const ssd_calibration &cal, const ssd_intrinsics *in);

/* the refusals a pass's host statement, its enqueue and its host-fed form share: the same text under each caller's name */
int check_gate_rule(const char *who, double k_sigma, double gate_min);
int check_clearance_rule(const std::string &who, const ssd_clearance_rule *rule);
int check_tread_grid_rule(const std::string &who, const ssd_tread_grid_rule *rule);
int check_pose_rule(const std::string &me, const ssd_stair_pose_rule *rule);
int check_fuse_rule(const std::string &me, int n, const ssd_depth_fuse_rule *rule, ssd_depth_fuse_rule *use);
int check_edge_rule(const std::string &me, const ssd_depth_edge_rule *rule, ssd_depth_edge_rule *use);
int check_warp_views(const std::string &me, const ssd_depth_warp_view *views, int nviews, const ssd_intrinsics *dst);
int check_fill_rule(const std::string &me, const ssd_depth_fill_rule *rule, ssd_depth_fill_rule *use);
int check_pose_targets(const std::string &me, const ssd_stair_pose_target *targets, int ntargets, const uint16_t *target_of_frame, int nframes, int input);

int pose_fold_frames(const char *who, const ssd_stair_pose_moments *records, const int *index, int nframes, std::vector<ssd_stair_pose_moments> &folds);

#pragma GCC visibility pop

#endif
