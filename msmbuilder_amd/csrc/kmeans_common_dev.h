// kmeans_common_dev.h -- what every k-means kernel shares: the workgroup size, the argument block KmArgsT and the final
// pick of a row (included by the kmeans_*_dev.h headers of kmeans.hip).
#pragma once
#include "common.h"

namespace msm {

constexpr int KNT = 256;   // threads per workgroup of every k-means kernel

template <typename T>   // T = float (fp32 MFMA labelling) or double (fp64 MFMA labelling: scikit-learn keeps float64 input in float64)
struct KmArgsT {
    const T* X;             // [n, m] (or gathered batch)
    const msm_idx_t* rows;  // optional row gather (batch indices), else nullptr
    long long n, m, K;
    const T* C;             // device [K, m]
    const T* cnorm;         // device [K]
    int32_t* labels;        // [n]
    // centre-split launch (small batches): blockIdx.y owns centre tiles [y*jspan, (y+1)*jspan) and
    // writes its (min value, index) candidates to pv/pi [gridDim.y][n]; a reduce kernel finishes
    long long jspan;        // 0 = all centres in one workgroup
    int xcd_ns;             // > 0 (kmeans_label_v4_kernel, large n): a 1-D grid of ceil(rowblocks / 8) x 8 x xcd_ns workgroups in
                            // which the xcd_ns centre splits of a row block are CONSECUTIVE workgroups of one XCD (see the kernel)
    T* pv;
    int* pi;
    const int* stop;        // optional device flag: non-zero -> the launch does nothing (msm_mbk_run: steps queued
                            // behind the one at which the convergence criterion fired)
};

// end of every label kernel: row i's pick between the two centre halves of its workgroup (lowest value, then lowest
// index), written as the split launch's candidate or as the label
template <typename T>
__device__ __forceinline__ void km_write_row(const KmArgsT<T>& P, long long i, T v0, T v1, int i0, int i1, int split)
{
    const bool second = (v1 < v0 || (v1 == v0 && i1 < i0));
    int lab = second ? i1 : i0;
    if (P.jspan) {
        P.pv[(long long)split * P.n + i] = second ? v1 : v0;
        P.pi[(long long)split * P.n + i] = lab;
    } else {
        if (lab == 0x7fffffff) lab = 0;  // all-NaN row: sklearn's argmin returns 0
        P.labels[i] = lab;
    }
}

}  // namespace msm
