// ba_host_shared.inc -- the host steps that the single-window path (ba_single_host.inc) and the window-batched path (ba_windows_host.inc) must do
// alike: Huber threshold, pose staging, the early exits, unpacking a result block.  Included by opt.hip before both.

static double ba_now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// thHuberMono = sqrt(5.991) (LocalBundleAdjustment) / thHuber2D = sqrt(5.99) (merge window, global BA), float constants upstream
static double ba_huber_delta(int mode) { return mode == 0 ? (double)(float)std::sqrt(5.991) : (double)(float)std::sqrt(5.99); }

// the caller's poses [qx qy qz qw tx ty tz] as the kernels read them: eight doubles a key-frame
static void ba_stage_poses(int32_t nKF, const float *kf_pose7, double *T0) {
    for (int k = 0; k < nKF; k++) {
        const DSE3 P = se3_from_float7(kf_pose7 + (size_t)k * 7);
        double *t = T0 + (size_t)k * 8;
        t[0] = P.r.x; t[1] = P.r.y; t[2] = P.r.z; t[3] = P.r.w; t[4] = P.t.x; t[5] = P.t.y; t[6] = P.t.z; t[7] = 0;
    }
}

// Zeroes `stats` and takes the reference's exits before any device work.  true: the window ends here with status *rc.
static bool ba_early_exit(int mode, int32_t nKF, const uint8_t *kf_fixed, const volatile uint8_t *stop_flag, int32_t *stats, int *rc) {
    *rc = RUMI_OK;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    int nFixed = 0;
    for (int k = 0; k < nKF; k++) nFixed += kf_fixed[k] ? 1 : 0;
    if (nFixed == 0 && mode == 0) { g_lastError = "LM-LBA: There are 0 fixed KF in the optimizations, LBA aborted"; *rc = RUMI_E_INVALID; return true; }   // Optimizer.cc:1057-1060
    if (mode != 2 && stop_flag && *stop_flag) { if (stats) stats[3] = 1; return true; }                                          // :1274-1276 / :3982-3984
    return false;
}

// A result block [T | X | erase] as it came back from the device -> the caller's arrays (fixed key-frames keep their input pose)
static void ba_unpack(int32_t nKF, const uint8_t *kf_fixed, int32_t nMP, int32_t nE, const double *T1, const double *X1, const uint8_t *erase,
                      float *kf_pose7, float *mp_pos3, uint8_t *erase_out) {
    if (nE > 0) std::memcpy(erase_out, erase, (size_t)nE);
    for (int k = 0; k < nKF; k++) {
        if (kf_fixed[k]) continue;
        const double *t = T1 + (size_t)k * 8;
        se3_to_float7(DSE3{{t[0], t[1], t[2], t[3]}, {t[4], t[5], t[6]}}, kf_pose7 + (size_t)k * 7);
    }
    for (size_t i = 0; i < (size_t)nMP * 3; i++) mp_pos3[i] = (float)X1[i];
}
// the four words of `stats` after a run (the merge BA reports its two passes apart)
static void ba_write_stats(int mode, int iters, int itersFirst, int trials, int nOpt, int32_t *stats) {
    if (stats) { stats[0] = mode == 1 ? itersFirst : iters; stats[1] = trials; stats[2] = nOpt; stats[3] = mode == 1 ? iters - itersFirst : 0; }
}
