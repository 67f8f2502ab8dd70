// tds_rb_internal.h — the handle behind tds_rb_sim_t, shared by tds_rb.hip (stepping), tds_rb_diff.hip (forward-mode
// rollout derivatives) and tds_rb_vjp.hip (reverse mode).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "tds_hip.h"
#include "tds_rb_step.h"

struct tds_rb_sim {
  tds_rb_model_t model;
  int num_worlds = 0, device = 0, dtype = TDS_DTYPE_F64;
  size_t elem = 8;
  hipStream_t stream = nullptr;
  void *d_state = nullptr, *d_model = nullptr;
  RbDev<double> h64;
  RbDev<float> h32;
  std::vector<float> stage;
  // tds_rb_jvp: tangents of the launch's lanes; tds_rb_vjp: state store, tapes and adjoints.  Grown as needed, kept for
  // the next call
  void *d_work = nullptr;
  size_t work_bytes = 0;
};

// sets tds_rb_last_error's message (tds_rb.hip); returns code
int tds_rb_fail(int code, const char *msg);
