// The parametric-head object of flame_out.hip, shared with flame_fit.hip (the fit runs the forward's own kernels on the object's tables
// and scratch).  Host side only.
#pragma once
#include <vector>

#include "../../include/fdm_hip.h"
#include "handoff.hpp"
#include "host.hpp"

struct fdm_flame : fdm::Handoff {         // lens: frames per clip
  int V = 0, J = 0, NB = 0, expr_at = 0, NL = 0, chunks = 0;
  std::vector<int> parents;
  float *D = nullptr, *T = nullptr, *JT = nullptr, *JD = nullptr, *wts = nullptr, *lb = nullptr;   // device: the model
  int *par = nullptr, *lv = nullptr;
  float *xf = nullptr, *pf = nullptr, *cf = nullptr, *vid = nullptr;       // scratch of the call in flight
  long long xf_cap = 0, pf_cap = 0, cf_cap = 0, vid_cap = 0;
};

namespace fdm {
// the forward's first two launches, on the object's tables and scratch (grown by the caller; F->lens holds the call's clip lengths)
void flame_launch_pose(fdm_flame* F, const float* shape, int shape_rows, int NS, const float* expr, int NE, const float* pose, int L_max, long long rows,
                       hipStream_t s);
void flame_launch_shape(fdm_flame* F, const float* shape, int NS, int shape_rows, hipStream_t s);
}  // namespace fdm
