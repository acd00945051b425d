// pose_opt_host.inc -- host side of PoseOptimization (kernel: pose_opt.inc): the device-resident entry the tracker calls and the two C entries.
// Included by opt.hip.

namespace rumi {
int pose_opt_device(const int32_t *dStart, const float *dXw, const float *dObs, const float *dW, const float *dK4, const float *dTin, float *dTout,
                    uint8_t *dOutlier, int32_t *dNGood, uint8_t *dActive, double *dLastChi2, bool fitsLds, hipStream_t st, int nbatch) {
    const PoseArgs A{dStart, dXw, dObs, dW, dK4, dTin, dTout, dOutlier, dNGood, dActive, dLastChi2, 1};
    // the frames' sizes are known to the device only: both instantiations are launched, the one a size does not belong to returns at once
    hipLaunchKernelGGL((k_pose_opt<true, 256>), dim3(nbatch), dim3(256), 0, st, A);
    if (!fitsLds) hipLaunchKernelGGL((k_pose_opt<false, 256>), dim3(nbatch), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? RUMI_OK : RUMI_E_NO_DEVICE;
}
}  // namespace rumi

extern "C" int rumi_pose_optimization_batch(RumiOptimizer *o, int32_t nbatch, const int32_t *start, const float *Xw, const float *obs,
                                            const float *inv_sigma2, const float *K4, float *Tcw7, uint8_t *outlier_out,
                                            int32_t *n_good_out) {
    if (!o || nbatch < 1 || !start || !K4 || !Tcw7 || !n_good_out) return RUMI_E_INVALID;
    const int total = start[nbatch];
    if (nbatch > o->pose.maxBatch || total > o->pose.maxEdges) { g_lastError = "pose optimisation: batch larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    if (total > 0 && (!Xw || !obs || !inv_sigma2 || !outlier_out)) return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(o->device));
    // one pinned block up: [start | K4 | T | Xw | obs | w]; one block back: [nGood | T | outlier]
    const size_t oStart = 0, oK = al16(oStart + (size_t)(nbatch + 1) * 4), oT = al16(oK + 16), oX = al16(oT + (size_t)nbatch * 28),
                 oO = al16(oX + (size_t)total * 12), oW = al16(oO + (size_t)total * 8), inBytes = al16(oW + (size_t)total * 4);
    const size_t rG = 0, rT = al16(rG + (size_t)nbatch * 4), rO = al16(rT + (size_t)nbatch * 28), outBytes = al16(rO + (size_t)total);
    uint8_t *hs = o->pose.in.h;
    std::memcpy(hs + oStart, start, (size_t)(nbatch + 1) * 4);
    std::memcpy(hs + oK, K4, 16);
    std::memcpy(hs + oT, Tcw7, (size_t)nbatch * 28);
    if (total > 0) {
        std::memcpy(hs + oX, Xw, (size_t)total * 12); std::memcpy(hs + oO, obs, (size_t)total * 8); std::memcpy(hs + oW, inv_sigma2, (size_t)total * 4);
    }
    HIP_TRY(hipMemcpyAsync(o->pose.in.d, hs, inBytes, hipMemcpyHostToDevice, nullptr));
    uint8_t *di = o->pose.in.d, *dout = o->pose.out.d;
    PoseArgs A{(const int32_t *)(di + oStart), (const float *)(di + oX), (const float *)(di + oO), (const float *)(di + oW), (const float *)(di + oK),
               (const float *)(di + oT), (float *)(dout + rT), dout + rO, (int32_t *)(dout + rG), o->pose.active.p, o->pose.lastChi2.p, 1};
    bool anyBig = false, anySmall = false;
    for (int b = 0; b < nbatch; b++) { const int nb = start[b + 1] - start[b]; anyBig |= nb > kPoseLdsEdges; anySmall |= nb <= kPoseLdsEdges; }
    // 256 threads per frame: measured against 128 (216 us for one frame of 300 correspondences) and 512 (265 us) it is the fastest (194 us)
    if (anySmall) hipLaunchKernelGGL((k_pose_opt<true, 256>), dim3(nbatch), dim3(256), 0, nullptr, A);
    if (anyBig) hipLaunchKernelGGL((k_pose_opt<false, 256>), dim3(nbatch), dim3(256), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(o->pose.out.h, dout, outBytes, hipMemcpyDeviceToHost));
    std::memcpy(n_good_out, o->pose.out.h + rG, (size_t)nbatch * 4);
    std::memcpy(Tcw7, o->pose.out.h + rT, (size_t)nbatch * 28);           // early returns (< 3 correspondences) carry the input pose
    if (total > 0) std::memcpy(outlier_out, o->pose.out.h + rO, (size_t)total);
    return RUMI_OK;
}

extern "C" int rumi_pose_optimization(RumiOptimizer *o, const float *Xw, const float *obs, const float *inv_sigma2, int32_t n,
                                      const float *K4, float *Tcw7, uint8_t *outlier_out, int32_t *n_good_out) {
    if (n < 0) return RUMI_E_INVALID;
    const int32_t start[2] = {0, n};
    return rumi_pose_optimization_batch(o, 1, start, Xw, obs, inv_sigma2, K4, Tcw7, outlier_out, n_good_out);
}
