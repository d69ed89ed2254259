// Contract between the row-pass code object of a row-only model (csrc/inflx_rowpass_kernels.hip, `<artefact>.rowpass`) and
// libinflx_hip.so.  Plain C types only.
#pragma once
#include <stdint.h>

#include "inflx_kernel_abi.h"

#define INFLX_ROWPASS_ABI_VERSION 1u
#define INFLX_INLINE_PARAMS 16  // doubles of parameters a sweep may carry in InflxRowPassArgs::params_inline

// Launch arguments of inflx_rowpass_*: those of inflx_sweep_rowvals_* (grid.x = 64-row blocks, grid.y = parameter rows) plus
//   grid.z = write slices -- workgroups that evaluate the same 64 rows and share their table region;
//   params_inline -- when `a.params` is NULL the P parameter rows travel here (P * N_PARAMETERS <= INFLX_INLINE_PARAMS): a
//   single-batch sweep then needs no parameter slot, no upload and no release event.
struct InflxRowPassArgs {
  struct InflxSweepArgs a;
  double params_inline[INFLX_INLINE_PARAMS];
};
