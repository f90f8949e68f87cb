// series_run.h -- how abi_series.hip starts the kernels of series.hip.  Internal.
#ifndef SPERR_AMD_SERIES_RUN_H
#define SPERR_AMD_SERIES_RUN_H

#include "common.h"
#include "series.h"

namespace sperrhip {

// The tables are device arrays with one entry per step (band) of the WHOLE series of nsteps steps; the launches cover
// the groups [g0, g1) of its plan, one launch per run of consecutive groups of one l.  Every volume holds n samples.
// d_steps: floats or doubles; d_bands: doubles
int series_forward_run(const void* const* d_steps, int is_float, double* const* d_bands, size_t nsteps, int levels,
                       size_t g0, size_t g1, size_t n, hipStream_t st);
// a NULL band counts as zero, a NULL output is not written
int series_inverse_run(const double* const* d_bands, void* const* d_outs, int output_float, size_t nsteps, int levels,
                       size_t g0, size_t g1, size_t n, hipStream_t st);

}  // namespace sperrhip

#endif
