// A model being trained (todhip_model of include/todhip.h): shared by train.hip, which fills it, and model_compact.hip, which thins it.
#pragma once

#include "ctx.h"

// desc: cap x 32 bytes, pts: cap x 3 f32; small[0] = the model's rows (device-resident: no call needs it on the host to append),
// small[1] = rows added by the last call, small[2] = the last observation's keypoints. The rest is scratch, which only grows: one
// observation's (img, mask, er_tmp, er and depth are the single-view call's alone), or a batch's -- todhip_model_add_observations_device
// keeps view v's keypoints, flags and points at row v * n_features of kp_*, flags and offs, the views' cameras in cams and
// the per-view totals, bases and added rows in batch (train.hip: BatchWords).
constexpr uint32_t kTrainBatchMaxViews = 64;
struct todhip_model {
  DevBuf desc, pts, kp_xy, kp_aux, kp_desc, img, mask, er_tmp, er, depth, flags, offs, small, cams, batch;
  uint32_t cap = 0;
};
