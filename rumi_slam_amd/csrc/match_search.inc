// The matcher's host search pipeline -- candidate lists, resolve, results, with the retries an overflowing list asks for -- and the C entries
// built on it.
namespace rumi {

// count pass, scan, fill pass.  The fill pass refuses to write past the list arena and raises the overflow word instead; the
// caller sees it in the result block, grows the arena and repeats the call (search_loop) — no mid-pipeline read-back.
int build_lists(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, bool retry, bool fused) {
    FLUSH(m);
    if (retry) HIP_TRY(hipMemsetAsync(m->dOut, 0, 4 * sizeof(int32_t), nullptr));   // the first attempt's header was cleared with the frame upload
    if (nq > 0 && fused) {
        // one launch: every query's list in a fixed slot of the arena (k_candidates<2>)
        const int slot = (int)std::min<size_t>(m->lists.cap / (size_t)nq, 0x7FFFFFFF / (size_t)nq);
        hipLaunchKernelGGL(k_candidates<2>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->lists.p, slot, m->dOverflow);
    } else if (nq > 0) {
        hipLaunchKernelGGL(k_candidates<0>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->lists.p, 0, m->dOverflow);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(256), 0, nullptr, nq, m->dCounts, m->dOffsets);
        hipLaunchKernelGGL(k_candidates<1>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->lists.p, (int)std::min<size_t>(m->lists.cap, 0x7FFFFFFF), m->dOverflow);
    }
    return RUMI_OK;
}

// bring back [header | featMp | assign] with one copy (synchronises the null stream); hOut[1] is then the overflow word of the candidate lists
static int fetch_results(RumiMatcher *m, int nfeat, int nq, bool wantAssign) {
    const size_t ints = wantAssign ? (size_t)4 + m->maxFeat + std::max(nq, 0) : (size_t)4 + std::max(nfeat, 0);
    HIP_TRY(hipMemcpy(m->hOut, m->dOut, ints * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RUMI_OK;
}

// Candidate lists, the resolve (`resolve()` launches it on the arrays as they are at that moment: the arena may have moved) and the results, until
// the overflow word comes back clear.  fused: first with every query's list in a fixed slot (one candidate launch); a query that does not fit
// falls back to count / scan / fill, which sizes the lists exactly; an arena too small for those is grown, once.
template <class Resolve>
static int search_loop(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, bool fused, bool wantAssign, Resolve resolve) {
    for (int attempt = 0, grown = 0; attempt < 4; attempt++) {
        RC_TRY(build_lists(m, mode, nq, fd, dQueryDesc, attempt > 0, fused));
        resolve();
        HIP_TRY(hipGetLastError());
        RC_TRY(fetch_results(m, fd.n, nq, wantAssign));
        if (m->hOut[1] == 0) break;
        if (m->hOut[1] == kFusedOverflow) { fused = false; continue; }      // the resolve did not run; repeat with exact list sizes
        // list arena too small: the resolve did not run and the frame's map-point vector is untouched
        if (grown) { g_lastError = "candidate list arena overflow after growing"; return RUMI_E_CAPACITY; }
        RC_TRY(m->lists.reserve((size_t)m->hOut[1], (size_t)m->hOut[1] * 2));
        grown = 1;
    }
    return RUMI_OK;
}

int run_search(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, const int32_t *dMpObs, float nnratio, int checkOri,
               int32_t *hostFeatMp, int32_t *nmatchesOut, const uint8_t *dBlocked0, float thrF, int thrI, int32_t *hostAssign) {
    const bool fused = track_speculation().fused && nq > 0 && m->lists.cap / (size_t)nq >= 64;
    RC_TRY(search_loop(m, mode, nq, fd, dQueryDesc, fused, hostAssign != nullptr, [&] {
        const ResolveArgs A{mode, nq, fd.n, m->dQ, m->dCounts, m->dOffsets, m->lists.p, fd.keys, dMpObs, m->dFeatMp, m->dAssign, m->dNmatches,
                            nnratio, checkOri, dBlocked0, thrF, thrI, m->dOverflow};
        launch_resolve(A, nullptr);
    }));
    *nmatchesOut = m->hOut[0];
    if (fd.n > 0 && hostFeatMp) std::memcpy(hostFeatMp, m->hOut + 4, (size_t)fd.n * sizeof(int32_t));
    if (nq > 0 && hostAssign) std::memcpy(hostAssign, m->hOut + 4 + m->maxFeat, (size_t)nq * sizeof(int32_t));
    return RUMI_OK;
}

// The candidate points of SearchByProjection(KF, Sim3) and Fuse, their pose pack and their queries (k_queries_sim3)
static int stage_sim3_queries(RumiMatcher *m, const FrameDev &fd, int nlevels, float logScaleFactor, const float *Tcw7, const float *Ow3, const float *K4, int nmp,
                              const uint8_t *skip, const float *pos, const float *normal, const float *minDist, const float *maxDist, const uint8_t *desc,
                              float th, int variant, int blocks, int checkReproj) {
    RC_TRY(stage_pose_ow(m, Tcw7, K4, Ow3));
    if (nmp > 0) {
        H2D(m->dU8a, skip, nmp); H2D(m->dF[0], pos, (size_t)nmp * 3); H2D(m->dF[1], normal, (size_t)nmp * 3);
        H2D(m->dF[2], minDist, nmp); H2D(m->dF[3], maxDist, nmp); H2D(m->dQDesc, desc, (size_t)nmp * 32);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_sim3, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dU8a, m->dF[0], m->dF[1], m->dF[2], m->dF[3],
                           m->dPose, m->dScale, nlevels, logScaleFactor, th, variant, blocks, checkReproj, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    }
    return RUMI_OK;
}

}  // namespace rumi

extern "C" int rumi_search_by_projection_mappoints(RumiMatcher *m, const RumiFrameFeatures *F, int32_t nmp,
                                                   const uint8_t *track_in_view, const float *proj_x, const float *proj_y,
                                                   const int32_t *scale_level, const float *view_cos, const float *track_depth,
                                                   const uint8_t *is_bad, const uint8_t *mp_desc, const int32_t *mp_obs, float th,
                                                   int32_t far_points, float th_far_points, float nnratio, int32_t *frame_mp,
                                                   int32_t *nmatches_out) {
    if (!m || !nmatches_out || !frame_mp || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, F, &fd));
    if (F->n > 0) H2D(m->dFeatMp, frame_mp, F->n);
    if (nmp > 0) {
        H2D(m->dU8a, track_in_view, nmp); H2D(m->dU8b, is_bad, nmp);
        H2D(m->dF[0], proj_x, nmp); H2D(m->dF[1], proj_y, nmp); H2D(m->dF[2], view_cos, nmp); H2D(m->dF[3], track_depth, nmp);
        H2D(m->dI[0], scale_level, nmp); H2D(m->dI[1], mp_obs, nmp);
        H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_mappoints, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dU8a, m->dF[0], m->dF[1],
                           m->dI[0], m->dF[2], m->dF[3], m->dU8b, m->dI[1], m->dScale, th, far_points, th_far_points, m->dQ);
    }
    return run_search(m, MODE_MAPPOINTS, nmp, fd, m->dQDesc, m->dI[1], nnratio, 0, frame_mp, nmatches_out);
}

extern "C" int rumi_search_by_projection_frame(RumiMatcher *m, const RumiFrameFeatures *Cur, const float *Tcw7, const float *K4,
                                               const RumiKeyPoint *last_keys, int32_t nlast, const int32_t *last_mp,
                                               const uint8_t *last_outlier, int32_t nmp, const float *mp_pos, const uint8_t *mp_desc,
                                               const int32_t *mp_obs, float th, int32_t check_orientation, int32_t *cur_mp,
                                               int32_t *nmatches_out) {
    if (!m || !nmatches_out || !cur_mp || nlast < 0 || nmp < 0 || !Tcw7 || !K4) return RUMI_E_INVALID;
    if (nlast > m->maxQ || nmp > m->maxQ) { g_lastError = "more last-frame features / map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, Cur, &fd));
    if (Cur->n > 0) H2D(m->dFeatMp, cur_mp, Cur->n);
    RC_TRY(stage_pose(m, Tcw7, K4));
    if (nmp > 0) { H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dI[1], mp_obs, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32); }
    RC_TRY(stage_last_frame(m, last_keys, nlast, last_mp, last_outlier));
    if (nlast > 0) {
        FLUSH(m);
        launch_queries_frame(m, fd, nlast, th, nullptr);
    }
    return run_search(m, MODE_FRAME, nlast, fd, m->dQDesc, m->dI[1], 0.f, check_orientation, cur_mp, nmatches_out);
}

extern "C" int rumi_search_by_bow(RumiMatcher *m, const RumiFrameFeatures *KF, const RumiFeatureVector *kf_fv, const int32_t *kf_mp,
                                  int32_t nmp, const uint8_t *mp_bad, const RumiFrameFeatures *F, const RumiFeatureVector *f_fv,
                                  float nnratio, int32_t check_orientation, int32_t *matches, int32_t *nmatches_out) {
    if (!m || !KF || !kf_fv || !f_fv || !matches || !nmatches_out || nmp < 0 || !kf_mp) return RUMI_E_INVALID;
    const int nqe = kf_fv->n_nodes > 0 ? kf_fv->offsets[kf_fv->n_nodes] : 0;     // one query per FeatureVector entry
    const int nfe = f_fv->n_nodes > 0 ? f_fv->offsets[f_fv->n_nodes] : 0;
    if (KF->n > m->maxQ || nqe > m->maxQ || nmp > m->maxQ || kf_fv->n_nodes > m->maxQ || nfe > m->maxFeat || f_fv->n_nodes > m->maxFeat) {
        g_lastError = "SearchByBoW: sizes exceed the matcher's capacities";
        return RUMI_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, F, &fd));
    RC_TRY(stage_query_keyframe(m, KF, kf_mp));
    if (nmp > 0) H2D(m->dU8a, mp_bad, nmp);
    RC_TRY(stage_fv_query(m, kf_fv, nqe));
    RC_TRY(stage_fv_frame(m, f_fv, nfe));
    m->gridPending = false;                                 // candidates come from the FeatureVectors: the spatial grid is not read
    FLUSH(m);
    if (kf_fv->n_nodes > 0) launch_queries_bow(m, nqe, kf_fv->n_nodes, f_fv->n_nodes, nullptr, nullptr);
    return run_search(m, MODE_BOW, nqe, fd, m->dQDesc, nullptr, nnratio, check_orientation, matches, nmatches_out);
}

extern "C" int rumi_search_by_bow_kf(RumiMatcher *m, const RumiFrameFeatures *KF1, const RumiFeatureVector *fv1, const int32_t *kf1_mp,
                                     const RumiFrameFeatures *KF2, const RumiFeatureVector *fv2, const int32_t *kf2_mp, int32_t nmp,
                                     const uint8_t *mp_bad, float nnratio, int32_t check_orientation, int32_t *matches12,
                                     int32_t *nmatches_out) {
    if (!m || !KF1 || !KF2 || !fv1 || !fv2 || !kf1_mp || !kf2_mp || !matches12 || !nmatches_out || nmp < 0) return RUMI_E_INVALID;
    const int nqe = fv1->n_nodes > 0 ? fv1->offsets[fv1->n_nodes] : 0, nfe = fv2->n_nodes > 0 ? fv2->offsets[fv2->n_nodes] : 0;
    if (KF1->n > m->maxQ || nqe > m->maxQ || nmp > m->maxQ || fv1->n_nodes > m->maxQ || nfe > m->maxFeat || fv2->n_nodes > m->maxFeat) {
        g_lastError = "SearchByBoW(KF,KF): sizes exceed the matcher's capacities";
        return RUMI_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, KF2, &fd));
    // a KF2 feature is a candidate only if it holds a good map point (:732-736): everything else starts blocked
    std::vector<uint8_t> blocked(std::max(KF2->n, 1));
    for (int f = 0; f < KF2->n; f++) blocked[f] = kf2_mp[f] < 0 || kf2_mp[f] >= nmp || mp_bad[kf2_mp[f]];
    if (KF2->n > 0) H2D(m->dU8b, blocked.data(), KF2->n);
    RC_TRY(stage_query_keyframe(m, KF1, kf1_mp));
    if (nmp > 0) H2D(m->dU8a, mp_bad, nmp);
    RC_TRY(stage_fv_query(m, fv1, nqe));
    RC_TRY(stage_fv_frame(m, fv2, nfe));
    m->gridPending = false;
    FLUSH(m);
    if (fv1->n_nodes > 0) launch_queries_bow(m, nqe, fv1->n_nodes, fv2->n_nodes, nullptr, nullptr);
    std::vector<int32_t> assign(std::max(nqe, 1), -1);
    RC_TRY(run_search(m, MODE_BOW_KF, nqe, fd, m->dQDesc, nullptr, nnratio, check_orientation, nullptr, nmatches_out, m->dU8b, 0.f, 0, assign.data()));
    for (int i = 0; i < KF1->n; i++) matches12[i] = -1;
    for (int p = 0; p < nqe; p++) if (assign[p] >= 0) matches12[fv1->indices[p]] = assign[p];
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_sim3(RumiMatcher *m, const RumiFrameFeatures *KF, float log_scale_factor, const float *Tcw7,
                                              const float *Ow3, const float *K4, int32_t nmp, const uint8_t *skip, const float *mp_pos,
                                              const float *mp_normal, const float *mp_min_dist, const float *mp_max_dist,
                                              const uint8_t *mp_desc, int32_t th, float ratio_hamming, int32_t explicit_invz,
                                              int32_t *matched, int32_t *nmatches_out) {
    if (!m || !KF || !Tcw7 || !Ow3 || !K4 || !matched || !nmatches_out || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more candidate points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, KF, &fd));
    std::vector<uint8_t> blocked(std::max(KF->n, 1));
    for (int f = 0; f < KF->n; f++) blocked[f] = matched[f] != -1;                 // vpMatched[idx] != NULL (:442)
    if (KF->n > 0) { H2D(m->dU8b, blocked.data(), KF->n); H2D(m->dFeatMp, matched, KF->n); }
    RC_TRY(stage_sim3_queries(m, fd, KF->nlevels, log_scale_factor, Tcw7, Ow3, K4, nmp, skip, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, (float)th,
                              explicit_invz, 1, 0));
    return run_search(m, MODE_SIM3, nmp, fd, m->dQDesc, nullptr, 0.f, 0, matched, nmatches_out, m->dU8b, (float)RUMI_TH_LOW * ratio_hamming, 0);
}

extern "C" int rumi_fuse_candidates(RumiMatcher *m, const RumiFrameFeatures *KF, float log_scale_factor, const float *Tcw7, const float *Ow3,
                                    const float *K4, int32_t nmp, const uint8_t *skip, const float *mp_pos, const float *mp_normal,
                                    const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, float th,
                                    int32_t check_reprojection, int32_t *best_idx) {
    if (!m || !KF || !Tcw7 || !Ow3 || !K4 || nmp < 0 || (nmp > 0 && !best_idx)) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more candidate points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, KF, &fd));
    HIP_TRY(hipMemsetAsync(m->dU8b, 0, std::max(KF->n, 1), nullptr));              // nothing is blocked: the points do not compete
    RC_TRY(stage_sim3_queries(m, fd, KF->nlevels, log_scale_factor, Tcw7, Ow3, K4, nmp, skip, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, th, 0, 0,
                              check_reprojection));
    int32_t n = 0;
    return run_search(m, MODE_FUSE, nmp, fd, m->dQDesc, nullptr, 0.f, 0, nullptr, &n, m->dU8b, 0.f, RUMI_TH_LOW, best_idx);
}

static int sim3_direction(RumiMatcher *m, const RumiFrameFeatures *KF, float logSf, const float *K4, int n, const uint8_t *skip, const float *pc,
                          const float *mn, const float *mx, const uint8_t *desc, float th, int32_t *best) {
    for (int i = 0; i < n; i++) best[i] = -1;
    if (n == 0) return RUMI_OK;
    FrameDev fd;
    RC_TRY(upload_frame(m, KF, &fd));
    HIP_TRY(hipMemsetAsync(m->dU8b, 0, std::max(KF->n, 1), nullptr));
    H2D(m->dPose, K4, 4);
    H2D(m->dU8a, skip, n); H2D(m->dF[0], pc, (size_t)n * 3); H2D(m->dF[2], mn, n); H2D(m->dF[3], mx, n); H2D(m->dQDesc, desc, (size_t)n * 32);
    FLUSH(m);
    hipLaunchKernelGGL(k_queries_campoints, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, m->dU8a, m->dF[0], m->dF[2], m->dF[3], m->dPose, m->dScale,
                       KF->nlevels, logSf, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    int32_t cnt = 0;
    return run_search(m, MODE_FUSE, n, fd, m->dQDesc, nullptr, 0.f, 0, nullptr, &cnt, m->dU8b, 0.f, RUMI_TH_HIGH, best);
}

extern "C" int rumi_search_by_sim3(RumiMatcher *m, const RumiFrameFeatures *KF1, const RumiFrameFeatures *KF2, const float *K4,
                                   float log_scale_factor, const uint8_t *skip1, const float *pc1_in2, const float *min_dist1,
                                   const float *max_dist1, const uint8_t *desc1, const uint8_t *skip2, const float *pc2_in1,
                                   const float *min_dist2, const float *max_dist2, const uint8_t *desc2, float th, int32_t *match12,
                                   int32_t *nfound_out) {
    if (!m || !KF1 || !KF2 || !K4 || !nfound_out) return RUMI_E_INVALID;
    const int n1 = KF1->n, n2 = KF2->n;
    if (n1 < 0 || n2 < 0 || (n1 > 0 && (!skip1 || !pc1_in2 || !min_dist1 || !max_dist1 || !desc1 || !match12)) ||
        (n2 > 0 && (!skip2 || !pc2_in1 || !min_dist2 || !max_dist2 || !desc2)))
        return RUMI_E_INVALID;
    if (n1 > m->maxQ || n2 > m->maxQ) { g_lastError = "SearchBySim3: key-frame larger than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    std::vector<int32_t> vnMatch1(std::max(n1, 1)), vnMatch2(std::max(n2, 1));
    RC_TRY(sim3_direction(m, KF2, log_scale_factor, K4, n1, skip1, pc1_in2, min_dist1, max_dist1, desc1, th, vnMatch1.data()));
    RC_TRY(sim3_direction(m, KF1, log_scale_factor, K4, n2, skip2, pc2_in1, min_dist2, max_dist2, desc2, th, vnMatch2.data()));
    int nFound = 0;                                                                 // check agreement, :1480-1493
    for (int i1 = 0; i1 < n1; i1++) {
        match12[i1] = -1;
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) { match12[i1] = idx2; nFound++; }
    }
    *nfound_out = nFound;
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_reloc(RumiMatcher *m, const RumiFrameFeatures *Cur, float log_scale_factor, const float *Tcw7,
                                               const float *Ow3, const float *K4, const RumiKeyPoint *kf_keys, int32_t nkf,
                                               const int32_t *kf_mp, int32_t nmp, const uint8_t *skip, const float *mp_pos,
                                               const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, float th,
                                               int32_t orb_dist, int32_t check_orientation, int32_t *cur_mp, int32_t *nmatches_out) {
    if (!m || !Cur || !Tcw7 || !Ow3 || !K4 || !cur_mp || !nmatches_out || nkf < 0 || nmp < 0) return RUMI_E_INVALID;
    if (nkf > m->maxQ || nmp > m->maxQ) { g_lastError = "more key-frame features / map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, Cur, &fd));
    std::vector<uint8_t> blocked(std::max(Cur->n, 1));
    for (int f = 0; f < Cur->n; f++) blocked[f] = cur_mp[f] >= 0;                  // CurrentFrame.mvpMapPoints[i2] != NULL (:1746)
    if (Cur->n > 0) { H2D(m->dU8b, blocked.data(), Cur->n); H2D(m->dFeatMp, cur_mp, Cur->n); }
    RC_TRY(stage_pose_ow(m, Tcw7, K4, Ow3));
    if (nmp > 0) {
        H2D(m->dU8a, skip, nmp); H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
        H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
    }
    if (nkf > 0) {
        H2D(m->dQKeys, kf_keys, nkf); H2D(m->dI[0], kf_mp, nkf);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_reloc, dim3((nkf + 255) / 256), dim3(256), 0, nullptr, nkf, m->dQKeys, m->dI[0], m->dU8a, m->dF[0], m->dF[2],
                           m->dF[3], m->dPose, m->dScale, Cur->nlevels, log_scale_factor, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    }
    return run_search(m, MODE_RELOC, nkf, fd, m->dQDesc, nullptr, 0.f, check_orientation, cur_mp, nmatches_out, m->dU8b, 0.f, orb_dist);
}

extern "C" int rumi_search_for_initialization(RumiMatcher *m, const RumiFrameFeatures *F1, const RumiFrameFeatures *F2,
                                              float *prev_matched, int32_t window_size, float nnratio, int32_t check_orientation,
                                              int32_t *matches12, int32_t *nmatches_out) {
    if (!m || !F1 || !F2 || !nmatches_out || F1->n < 0) return RUMI_E_INVALID;
    if (F1->n > m->maxQ) { g_lastError = "more F1 key-points than max_queries"; return RUMI_E_CAPACITY; }
    if (F1->n > 0 && (!prev_matched || !matches12 || !F1->keys_un || !F1->desc)) return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, F2, &fd));
    const int n1 = F1->n;
    *nmatches_out = 0;
    if (n1 == 0) return RUMI_OK;
    H2D(m->dQKeys, F1->keys_un, n1); H2D(m->dQDesc, F1->desc, (size_t)n1 * 32); H2D(m->dF[0], prev_matched, (size_t)n1 * 2);
    FLUSH(m);
    hipLaunchKernelGGL(k_queries_init, dim3((n1 + 255) / 256), dim3(256), 0, nullptr, n1, m->dQKeys, m->dF[0], (float)window_size, m->dQ);
    RC_TRY(search_loop(m, MODE_INIT, n1, fd, m->dQDesc, false, true, [&] {          // (never the fused candidate pass)
        const InitArgs A{n1, fd.n, m->dQ, m->dCounts, m->dOffsets, m->lists.p, fd.keys, m->dAssign, m->dF[0], m->dNmatches, nnratio, check_orientation,
                         m->dOverflow};
        hipLaunchKernelGGL(k_resolve_init, dim3(1), dim3(64), (size_t)std::max(fd.n, 1) * 2 * sizeof(int32_t), nullptr, A);
    }));
    *nmatches_out = m->hOut[0];
    std::memcpy(matches12, m->hOut + 4 + m->maxFeat, (size_t)n1 * sizeof(int32_t));
    HIP_TRY(hipMemcpy(prev_matched, m->dF[0], (size_t)n1 * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return RUMI_OK;
}

extern "C" int rumi_frame_is_in_frustum(RumiMatcher *m, const float *Rcw9, const float *tcw3, const float *Ow3, const float *K4,
                                        float min_x, float min_y, float max_x, float max_y, float log_scale_factor, int32_t nlevels,
                                        float viewing_cos_limit, int32_t nmp, const float *mp_pos, const float *mp_normal,
                                        const float *mp_min_dist, const float *mp_max_dist, uint8_t *track_in_view, float *proj_x,
                                        float *proj_y, int32_t *scale_level, float *view_cos, float *track_depth) {
    if (!m || !Rcw9 || !tcw3 || !Ow3 || !K4 || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;
    if (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !track_in_view || !proj_x || !proj_y || !scale_level || !view_cos || !track_depth)
        return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    reset_uploads(m);
    RC_TRY(stage_pose_matrices(m, Rcw9, tcw3, Ow3, K4));
    H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
    // outputs are packed into the upload mirror (its contents have been scattered by then) and come back with one copy
    if (!frustum_fits(m, nmp)) { g_lastError = "isInFrustum: result block exceeds the staging block"; return RUMI_E_CAPACITY; }
    const FrustumBlock fb(m->stage.d, nmp);
    FLUSH(m);
    hipLaunchKernelGGL(k_is_in_frustum, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dPose, min_x, min_y, max_x, max_y, log_scale_factor,
                       nlevels, viewing_cos_limit, m->dF[0], m->dF[1], m->dF[2], m->dF[3], fb.inView, fb.x, fb.y, fb.level, fb.viewCos, fb.depth);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(m->stage.h, m->stage.d, fb.bytes, hipMemcpyDeviceToHost));
    FrustumBlock(m->stage.h, nmp).unpack(nmp, track_in_view, proj_x, proj_y, scale_level, view_cos, track_depth);
    return RUMI_OK;
}

extern "C" int rumi_search_local_points(RumiMatcher *m, const RumiFrameFeatures *F, const float *Rcw9, const float *tcw3, const float *Ow3,
                                        const float *K4, float log_scale_factor, int32_t nlevels, float viewing_cos_limit, int32_t nmp,
                                        const uint8_t *skip, const float *mp_pos, const float *mp_normal, const float *mp_min_dist,
                                        const float *mp_max_dist, const uint8_t *mp_desc, const int32_t *mp_obs, float th, int32_t far_points,
                                        float th_far_points, float nnratio, uint8_t *track_in_view, float *proj_x, float *proj_y,
                                        int32_t *scale_level, float *view_cos, float *track_depth, int32_t *n_to_match_out, int32_t *frame_mp,
                                        int32_t *nmatches_out) {
    if (!m || !F || !Rcw9 || !tcw3 || !Ow3 || !K4 || !nmatches_out || !n_to_match_out || !frame_mp || nmp < 0) return RUMI_E_INVALID;
    *nmatches_out = 0; *n_to_match_out = 0;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;                          // nToMatch == 0: the reference does not search (Tracking.cc:3032)
    if (!skip || !mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc || !mp_obs || !track_in_view || !proj_x || !proj_y || !scale_level ||
        !view_cos || !track_depth)
        return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    RC_TRY(upload_frame(m, F, &fd));
    if (F->n > 0) H2D(m->dFeatMp, frame_mp, F->n);
    RC_TRY(stage_pose_matrices(m, Rcw9, tcw3, Ow3, K4));
    H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
    H2D(m->dU8b, skip, nmp); H2D(m->dI[1], mp_obs, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
    // the frustum test writes the six per-point fields into the (by then scattered) upload mirror; the query kernel reads them there and the
    // same block travels back to the host for the facade's write-back: no host round trip between isInFrustum and SearchByProjection
    if (!frustum_fits(m, nmp)) { g_lastError = "SearchLocalPoints: result block exceeds the staging block"; return RUMI_E_CAPACITY; }
    const FrustumBlock fb(m->stage.d, nmp);
    FLUSH(m);
    hipLaunchKernelGGL(k_is_in_frustum, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dPose, fd.minX, fd.minY, fd.maxX, fd.maxY, log_scale_factor,
                       nlevels, viewing_cos_limit, m->dF[0], m->dF[1], m->dF[2], m->dF[3], fb.inView, fb.x, fb.y, fb.level, fb.viewCos, fb.depth, m->dU8b);
    HIP_TRY(hipMemcpyAsync(m->stage.h, m->stage.d, fb.bytes, hipMemcpyDeviceToHost, nullptr));
    // is_bad of SearchByProjection = skip: a skipped point is never in view, so the flag is only read for points that are not bad
    hipLaunchKernelGGL(k_queries_mappoints, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, fb.inView, fb.x, fb.y, fb.level, fb.viewCos, fb.depth, m->dU8b, m->dI[1],
                       m->dScale, th, far_points, th_far_points, m->dQ);
    RC_TRY(run_search(m, MODE_MAPPOINTS, nmp, fd, m->dQDesc, m->dI[1], nnratio, 0, frame_mp, nmatches_out));
    FrustumBlock(m->stage.h, nmp).unpack(nmp, track_in_view, proj_x, proj_y, scale_level, view_cos, track_depth);      // complete: run_search synchronised the stream
    int nTo = 0;
    for (int i = 0; i < nmp; i++) nTo += track_in_view[i];
    *n_to_match_out = nTo;
    if (nTo == 0) *nmatches_out = 0;                       // (nothing in view: no query was live, the search found nothing)
    return RUMI_OK;
}
