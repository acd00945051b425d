// k_assemble: the levels of a frame concatenated, the output slot of every key-point.  (Calls of a few frames do this in k_orient_desc's
// prologue instead: orb_orient_desc.inc.)
namespace rumi {

// Concatenate levels, assign slots: in (level, list) order, key-points with lap0 <= x*scale <= lap1 fill the
// output from the back (stereoIndex--), the others from the front (monoIndex++).
__global__ __launch_bounds__(256) void k_assemble(const DevParams *__restrict__ P, const uint32_t *__restrict__ selLevel,
                                                  const int32_t *__restrict__ selLevelCnt, int selLevelCap, int lap0,
                                                  int lap1, uint32_t *__restrict__ selPacked, uint32_t *__restrict__ selMeta,
                                                  int32_t *__restrict__ selCount, int selCap, int32_t *__restrict__ countsBase, long long countsStride,
                                                  int32_t *__restrict__ errFlag, int32_t *__restrict__ errMirror) {
    // errMirror (one-frame calls whose results go straight to pinned host memory): the call's error word is final when this workgroup ends -- every
    // kernel that can set a bit has run, the descriptor kernel sets none -- and is published beside the results: no copy of it follows
    __shared__ int lvStart[kMaxLevels + 1];
    __shared__ int part[256];
    const int tid = threadIdx.x, frame = blockIdx.x;
    int32_t *counts = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(countsBase) + frame * countsStride);   // {n, monoIndex} of this frame
    const int nl = P->nlevels;
    if (tid == 0) {
        int run = 0;
        for (int l = 0; l < nl; l++) { lvStart[l] = run; run += selLevelCnt[(long long)frame * nl + l]; }
        lvStart[nl] = run;
    }
    __syncthreads();
    const int total = lvStart[nl];
    if (total > selCap) {
        if (tid == 0) { selCount[frame] = 0; counts[0] = total; counts[1] = 0; const int old = atomicOr(errFlag, 8); if (errMirror) *errMirror = old | 8; }
        return;
    }
    const int chunk = (total + 255) / 256;
    const int k0 = tid * chunk, k1 = min(total, k0 + chunk);
    // pass 1: flags of my contiguous chunk
    int level = 0, nflag = 0;
    for (int k = k0; k < k1; k++) {
        while (k >= lvStart[level + 1]) level++;
        const uint32_t pk = selLevel[((long long)frame * nl + level) * selLevelCap + (k - lvStart[level])];
        float x = (float)((int)(pk & 0xFFF) + kBorder);
        if (level != 0) x = x * P->lv[level].scale;
        nflag += (x >= (float)lap0 && x <= (float)lap1) ? 1 : 0;
    }
    part[tid] = nflag;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; i++) { const int t = part[i]; part[i] = run; run += t; }
        selCount[frame] = total;
        counts[0] = total;
        counts[1] = total - run;      // monoIndex
        if (errMirror) *errMirror = *errFlag;
    }
    __syncthreads();
    int before = part[tid];                       // flagged key-points before k0
    level = 0;
    for (int k = k0; k < k1; k++) {
        while (k >= lvStart[level + 1]) level++;
        const uint32_t pk = selLevel[((long long)frame * nl + level) * selLevelCap + (k - lvStart[level])];
        float x = (float)((int)(pk & 0xFFF) + kBorder);
        if (level != 0) x = x * P->lv[level].scale;
        const bool f = x >= (float)lap0 && x <= (float)lap1;
        const int slot = f ? (total - 1 - before) : (k - before);
        before += f ? 1 : 0;
        selPacked[(long long)frame * selCap + k] = pk;
        selMeta[(long long)frame * selCap + k] = (uint32_t)level | ((uint32_t)slot << 8);
    }
}

void launch_assemble(const DevParams *dP, const uint32_t *selLevel, const int32_t *selLevelCnt, int selLevelCap, int lap0,
                     int lap1, uint32_t *selPacked, uint32_t *selMeta, int32_t *selCount, int selCap, int32_t *counts, long long countsStride,
                     int32_t *errFlag, int nframes, hipStream_t st, int32_t *errMirror) {
    hipLaunchKernelGGL(k_assemble, dim3(nframes), dim3(256), 0, st, dP, selLevel, selLevelCnt, selLevelCap, lap0, lap1,
                       selPacked, selMeta, selCount, selCap, counts, countsStride, errFlag, nframes == 1 ? errMirror : nullptr);
}

}  // namespace rumi
