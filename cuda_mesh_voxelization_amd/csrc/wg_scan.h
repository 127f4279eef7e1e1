// wg_scan.h -- workgroup-wide sums and scans shared by the compaction-shaped kernels (vox.hip, cvox.hip, extract.hip, components.hip,
// surfnets.hip).  Device inline templates only: the __global__ wrappers and their launches stay with the kernels that use them.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace vp {

// ---- one workgroup of exactly 1024 threads: exclusive scan of m values -----------------------------------------------------------
// put(i, sum of get(0 .. i)) for every i < m; returns the sum of all m values (0 for m = 0) to every thread.  Thread t serves the
// contiguous run [min(t per, m), min(t per + per, m)) with per = ceil(m / 1024): a serial sum, a Hillis-Steele scan of the 1024 sums in
// part[] (1024 elements of LDS from the caller), then a serial write-back, which calls get(i) a second time.  I is the index type of m.
// The barrier in front of the first store to part[] belongs to the function: a second call right behind the first one, with the same
// part[], never overwrites an element that a thread of the first call still has to read.
template <typename T, typename I, typename Get, typename Put>
__device__ __forceinline__ T wg_scan_1024(T* part, I m, Get get, Put put)
{
    const I tid = threadIdx.x;
    const I per = (m + 1023) / 1024;
    const I b = min(tid * per, m), e = min(b + per, m);
    T s = 0;
    for (I i = b; i < e; ++i) s += get(i);
    __syncthreads();
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const T v = tid >= (I)d ? part[tid - d] : T(0);
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    T run = part[tid] - s;
    for (I i = b; i < e; ++i) { put(i, run); run += get(i); }
    return part[1023];
}

// ---- workgroups of 256 threads (four waves), one value per thread ------------------------------------------------------------------
// Both take four elements of LDS from the caller and hold one barrier, between the store of the wave results to smem[] and the reads.
// smem[] may be reused once every thread is past those reads: the caller places a barrier before the next call that gets the same smem[].

// sum of v over the workgroup, returned to every thread
template <typename T>
__device__ __forceinline__ T wg_sum_256(T v, T* smem)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    return smem[0] + smem[1] + smem[2] + smem[3];
}

// sum of v over the threads before this one; total != nullptr: *total = the sum over the workgroup
template <typename T>
__device__ __forceinline__ T wg_exclusive_256(T v, T* smem, T* total = nullptr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) smem[wave] = incl;
    __syncthreads();
    T before = incl - v;
    for (int w = 0; w < wave; ++w) before += smem[w];
    if (total) *total = smem[0] + smem[1] + smem[2] + smem[3];
    return before;
}

}  // namespace vp
