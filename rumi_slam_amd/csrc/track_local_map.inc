// The point table of rumi_track_local_map, built on the device from the covisibility store's attribute records (included by track.hip; the
// store's side is covis.hip, the view between them covis_view.h).  Rows 0 .. n_local_points) are mvpLocalMapPoints in their order, then the
// frame's other points in order of their first feature, then the discarded outliers that have no row yet, in list order.
//
// rowOf[point] is a 64-bit stamp (epoch << 32) | value; a value of another epoch reads as "no row".  Inside an epoch
//   kRowBit | row          the point has its row: it compares above every claim, so a 64-bit atomicMax never replaces it
//   0x7FFFFFFF - u         candidate u claims the point (u = feature index, or n + place in the discarded list): the lowest u wins
//
//   k_table_mark     a lane per local point: its row is its place in the list
//   k_table_claim    a lane per candidate: atomicMax of its claim
//   k_table_extras   ONE workgroup: the winners in candidate order (block_ordered_slot, match_device.h), their rows; then the seen flags, the stale projections of
//                    the discarded outliers and the frame's vector translated from ids to rows
//   k_table_gather   table_gather_rows with every array: the rows written straight into the arrays the frustum test, the search and the optimiser read
// The stamps (table_stamp, table_claim, table_row, table_row_of) and table_gather_rows also serve the point table of a relocalisation session
// (track_reloc_resident.inc), which has a map and an epoch counter of its own.
// Integer work and copies only: the table does not depend on the order anything arrives in.

constexpr uint32_t kRowBit = 0x80000000u;
constexpr int kTableThreads = 1024;

struct TableArgs {
    CovisLocalView v;
    int rowCap;                          // rows the destination arrays hold: min(the tracker's max_points, table_cap)
    float *pos, *normal, *minDist, *maxDist;
    int32_t *obs;
    uint32_t *desc;
    uint8_t *bad, *local, *seen, *staleIn;
    float *staleProj;
    int32_t *featMp, *tableIds;
};

// ---- the vocabulary of an epoch-stamped point table: this one and the relocalisation session's (track_reloc_resident.inc) ----
__device__ __forceinline__ unsigned long long table_stamp(uint32_t epoch, uint32_t value) { return ((unsigned long long)epoch << 32) | value; }
__device__ __forceinline__ unsigned long long table_claim(uint32_t epoch, int u) { return table_stamp(epoch, 0x7FFFFFFFu - (uint32_t)u); }
__device__ __forceinline__ unsigned long long table_row(uint32_t epoch, int row) { return table_stamp(epoch, kRowBit | (uint32_t)row); }
__device__ __forceinline__ int table_row_of(const unsigned long long *rowOf, uint32_t epoch, int p) {
    const unsigned long long s = rowOf[p];
    return ((uint32_t)(s >> 32) == epoch && ((uint32_t)s & kRowBit)) ? (int)((uint32_t)s & ~kRowBit) : -1;
}

// The rows [0, nTable) of a table out of the store's records, by workgroups of 256 in a grid-stride loop over tiles of 256 rows: a lane per row for the
// scalar fields (the point record and two 16-byte loads of the attribute record), then eight lanes per row for the descriptor (a wave reads eight whole
// 32-byte rows).  FULL: normal, obs and local (row < nLocal) as well, which only the local-map table has.  A row without attributes reads as zeros.
struct TableRows { float *pos, *normal, *minDist, *maxDist; int32_t *obs; uint32_t *desc; uint8_t *bad, *local; };
template <bool FULL>
__device__ __forceinline__ void table_gather_rows(const CovisView &v, const int32_t *tableIds, int nTable, int nLocal, const TableRows &o) {
    __shared__ int sId[256];
    const int tid = threadIdx.x;
    for (int base = blockIdx.x * 256; base < nTable; base += gridDim.x * 256) {
        const int row = base + tid;
        int id = -1;
        if (row < nTable) {
            const int p = tableIds[row];
            const CovisPoint P = v.point(p);
            CovisAttrGeom A{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
            if (v.has_attr(P)) { id = p; A = v.attr_geom(p); }
            A.pos(o.pos + (size_t)row * 3);
            o.minDist[row] = A.min_dist(); o.maxDist[row] = A.max_dist();
            o.bad[row] = (uint8_t)P.bad();
            if (FULL) {
                A.normal(o.normal + (size_t)row * 3);
                o.obs[row] = P.obs_len();                    // Observations() of the monocular model: the length of the observer row
                o.local[row] = row < nLocal;
            }
        }
        sId[tid] = id;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int r = it * 32 + (tid >> 3), w = tid & 7;
            if (base + r < nTable) {
                const int p = sId[r];
                o.desc[(size_t)(base + r) * 8 + w] = p >= 0 ? (uint32_t)v.attr_desc(p)[w] : 0u;
            }
        }
        __syncthreads();
    }
}

// the candidate's point, or -1 when it asks for no row: NULL, or a bad point the frame holds (SearchLocalPoints' first loop drops it)
__device__ __forceinline__ int table_candidate(const TableArgs &a, int u) {
    const int p = u < a.v.nFrame ? a.v.framePts[u] : a.v.discIds[u - a.v.nFrame];
    if (p < 0) return -1;
    if (u < a.v.nFrame && a.v.t.point_bad(p)) return -1;
    return p;
}

__global__ __launch_bounds__(256) void k_table_mark(TableArgs a) {
    const int nLocal = a.v.head[3];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nLocal; j += gridDim.x * 256) {
        const int p = a.v.localPts[j];
        a.v.rowOf[p] = table_row(a.v.epoch, j);
        if (j < a.rowCap) { a.tableIds[j] = p; a.seen[j] = 0; }
        if (!a.v.t.has_attr(p)) atomicAdd(&a.v.head[5], 1);
    }
}

__global__ __launch_bounds__(256) void k_table_claim(TableArgs a) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.v.nFrame + a.v.nDiscarded) return;
    const int p = table_candidate(a, u);
    if (p >= 0) atomicMax(&a.v.rowOf[p], table_claim(a.v.epoch, u));
}

__global__ __launch_bounds__(kTableThreads) void k_table_extras(TableArgs a) {
    __shared__ int sCnt[kTableThreads / 64], sBase, sMissing;
    const int tid = threadIdx.x;
    const int n = a.v.nFrame, nd = a.v.nDiscarded, total = n + nd, nLocal = a.v.head[3];
    if (tid == 0) { sBase = 0; sMissing = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < total; c0 += kTableThreads) {
        const int u = c0 + tid;
        const int p = u < total ? table_candidate(a, u) : -1;
        const bool win = p >= 0 && a.v.rowOf[p] == table_claim(a.v.epoch, u);
        block_ordered_slot(win, sCnt, &sBase, [&](int slot) {
            const int row = nLocal + slot;
            a.v.rowOf[p] = table_row(a.v.epoch, row);
            if (row < a.rowCap) { a.tableIds[row] = p; a.seen[row] = 0; }
            if (u < n && !a.v.t.has_attr(p)) atomicAdd(&sMissing, 1);
        });
    }
    __threadfence_block();                                   // the rows written above are read below by other lanes of this workgroup
    __syncthreads();
    if (tid == 0) { a.v.head[4] = nLocal + sBase; if (sMissing) atomicAdd(&a.v.head[5], sMissing); }
    // the caller's discard loop first (2), then the frame's own points (1): rumi_track_local's order
    for (int k = tid; k < nd; k += kTableThreads) {
        const int row = table_row_of(a.v.rowOf, a.v.epoch, a.v.discIds[k]);
        if (row < 0 || row >= a.rowCap) continue;
        a.seen[row] = 2;
        if (a.v.discInView) {
            a.staleIn[row] = a.v.discInView[k];
            for (int j = 0; j < 5; j++) a.staleProj[(size_t)row * 5 + j] = a.v.discProj[(size_t)k * 5 + j];
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n; i += kTableThreads) {
        const int p = table_candidate(a, i);
        int row = p >= 0 ? table_row_of(a.v.rowOf, a.v.epoch, p) : -1;
        if (row >= a.rowCap) row = -1;                       // (the host refuses such a call: nothing of it is read)
        if (row >= 0) a.seen[row] = 1;
        a.featMp[i] = row;
    }
}

__global__ __launch_bounds__(256) void k_table_gather(TableArgs a) {
    table_gather_rows<true>(a.v.t, a.tableIds, min(a.v.head[4], a.rowCap), a.v.head[3],
                            TableRows{a.pos, a.normal, a.minDist, a.maxDist, a.obs, a.desc, a.bad, a.local});
}
