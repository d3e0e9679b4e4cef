// The lanes' speed limits as engine state (cfx_set_lane_speed_limits_device and its kin, include/cityflow_amd.h).
//
// The step reads a drivable's limit in one place per vehicle: DevNet::drvLM[d].y (cfx_kernels.h computeAction, the ring
// layout's kr_action / kl_action).  DevNet::drvMaxSpeed holds the same numbers unpacked.  Both arrays are the engine's own
// (cfx_engine::drvLM / drvMaxSpeed, non-const there), and only the kernels of this file write them after cfx_create — every
// write puts ONE value into both, so they can never disagree.  Lanes are the drivables [0, L); laneLinks are never touched.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

__device__ inline void putLaneLimit(double2 *drvLM, double *drvMaxSpeed, size_t l, double v) {
    drvLM[l].y = v;  // (the length beside it stays: an 8-byte store)
    drvMaxSpeed[l] = v;
}

// limits[l]: NaN keeps; finite and >= 0 is applied bit for bit; negative or infinite is left out and counted.  Grid-stride
// over the nLanes entries (all environments); the rejects of a wave are summed in registers and cost one atomic, and none
// where the wave has none.  `rejected` (null: not counted) was cleared ahead of the launch.
__global__ void k_set_lane_limits(const double *limits, int nLanes, double2 *drvLM, double *drvMaxSpeed, int32_t *rejected) {
    const size_t n = (size_t) nLanes, stride = (size_t) gridDim.x * blockDim.x;
    int bad = 0;
    for (size_t l = (size_t) blockIdx.x * blockDim.x + threadIdx.x; l < n; l += stride) {
        const double v = limits[l];
        if (v != v) continue;
        if (v >= 0.0 && v < __builtin_huge_val())
            putLaneLimit(drvLM, drvMaxSpeed, l, v);
        else
            ++bad;
    }
    if (!rejected) return;  // (uniform)
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(rejected, bad);
}

// the limits in force; every element of out[nLanes] is written
__global__ void k_get_lane_limits(int nLanes, const double *drvMaxSpeed, double *out) {
    const size_t n = (size_t) nLanes, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t l = (size_t) blockIdx.x * blockDim.x + threadIdx.x; l < n; l += stride) out[l] = drvMaxSpeed[l];
}

// the file's limits back in force, whatever they are (a file may hold what a set call would reject)
__global__ void k_restore_lane_limits(int nLanes, const double *fileLimits, double2 *drvLM, double *drvMaxSpeed) {
    const size_t n = (size_t) nLanes, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t l = (size_t) blockIdx.x * blockDim.x + threadIdx.x; l < n; l += stride) putLaneLimit(drvLM, drvMaxSpeed, l, fileLimits[l]);
}
