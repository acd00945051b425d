// The tables of an image size: set_geometry (the level records and resize tables of DevParams, then the tiles of the one-launch pyramid), and
// rumi_orb_tables.

// Step 1 of set_geometry: the level records of P from the host geometry, and the resize tables (column offsets and taps, row offsets and taps,
// the per-row table) the levels index into.
static void make_level_tables(const std::vector<LevelGeom> &g, DevParams &P, std::vector<int16_t> &coef, std::vector<RowTap> &rowTab) {
    for (int l = 0; l < P.nlevels; l++) {
        DevLevel &D = P.lv[l];
        const LevelGeom &G = g[l];
        D.w = G.w; D.h = G.h; D.pitch = G.pitch; D.off = G.off;
        D.nCols = G.nCols; D.nRows = G.nRows; D.wCell = G.wCell; D.hCell = G.hCell;
        D.cellBase = G.cellBase; D.nCells = G.nCells; D.maxBX = G.maxBX; D.maxBY = G.maxBY;
        D.nfeat = G.nfeat; D.scale = G.scale;
        D.patchSize = (float)(int)(kPatchSize * G.scale);
        D.candCap = std::min(G.candCap, 65535);
        D.coefX = D.coefXT = D.coefY = 0; D.xmax = D.xmaxFast = G.w; D.rowTab = 0;
        if (l > 0) {
            std::vector<int16_t> ofs, taps;
            int dmax;
            make_resize_axis(g[l - 1].w, G.w, true, ofs, taps, &dmax);
            D.coefX = (int)coef.size(); D.xmax = dmax;
            D.xmaxFast = dmax == G.w ? G.w + 3 : dmax;
            for (int k = 0; k < 4; k++) { ofs.push_back(ofs[G.w - 1]); taps.push_back(taps[2 * G.w - 2]); taps.push_back(taps[2 * G.w - 1]); }
            coef.insert(coef.end(), ofs.begin(), ofs.end());
            D.coefXT = (int)coef.size();
            coef.insert(coef.end(), taps.begin(), taps.end());
            make_resize_axis(g[l - 1].h, G.h, false, ofs, taps, &dmax);
            D.coefY = (int)coef.size();
            coef.insert(coef.end(), ofs.begin(), ofs.end());
            coef.insert(coef.end(), taps.begin(), taps.end());
            // per output row: the two clamped source rows (cv clips the ROW indices when it fetches them) and the taps << 16
            D.rowTab = (int)rowTab.size();
            const int sh = g[l - 1].h;
            for (int oy = 0; oy < G.h; oy++) {
                const int sy = ofs[oy];
                const int sy0 = sy >= 0 ? (sy < sh ? sy : sh - 1) : 0, sy1r = sy + 1, sy1 = sy1r >= 0 ? (sy1r < sh ? sy1r : sh - 1) : 0;
                rowTab.push_back(RowTap{sy0, sy1, (uint32_t)taps[oy * 2] << 16, (uint32_t)taps[oy * 2 + 1] << 16});
            }
        }
    }
}

// The batch quadtree's tables of a geometry (orb_octree.h): per level the coordinate halves of a key's depth-D path -- x half, then y half, by
// the rule the kernels share (oct_coord_bin) -- and where the level's depth-D cells lie in a frame's histogram / rank row.  A level whose
// aspect ratio gives no or too many roots has neither (its trees go to the kernel that reports that).
static void make_octree_tables(DevParams &P, std::vector<uint16_t> &bins) {
    bins.clear();
    int cells = 0;
    for (int l = 0; l < P.nlevels; l++) {
        DevLevel &D = P.lv[l];
        const int W = D.maxBX - kBorder, Hh = D.maxBY - kBorder;
        const OctLevelTabs T = oct_level_tabs(W, Hh, D.nfeat);
        D.octBin = (int)bins.size(); D.octCell = cells; D.octCells = T.cells;
        if (T.cells == 0) continue;
        bins.resize(bins.size() + (size_t)(W + 1 + Hh + 1));
        oct_make_bins(W, Hh, T, bins.data() + D.octBin);
        cells += oct_row_entries(T.cells);
    }
    P.octCellStride = cells;
}

// Step 2 of set_geometry: regions of the one-launch pyramid (k_pyramid_tiles): an even partition of the TOP level into tiles of about kPyrTX x kPyrTY pixels (16 x 8: 14.3 us for one 640 x 480 frame; 32 x 16: 19.4, 16 x 16: 16.5, 8 x 8: 15.1); going down, a tile's region of
// level l - 1 is the hull of what its region of level l reads (first tap column .. second tap column, first .. second source row) and of its
// share of an even partition of level l - 1 (every pixel of every level belongs to some tile); x ranges are widened to multiples of 4 (the
// kernels store dwords; the tables carry 4 padded columns).  Level 0's "region" is the window of the frame the tile reads.
// Small tiles for calls of a few frames, where the dependent chain is what counts (216 workgroups for one 640 x 480 frame).
constexpr int kPyrTX = 16, kPyrTY = 8;
static int build_pyramid_tiles(RumiOrb *h, const std::vector<int16_t> &coef, const std::vector<RowTap> &rowTab) {
    const DevParams &P = h->hP;
    h->nPyrTiles = 0; h->pyrBuf = 0;
    if (P.nlevels < 2) return RUMI_OK;
    const int top = P.nlevels - 1;
    const int ntx = (P.lv[top].w + kPyrTX - 1) / kPyrTX, nty = (P.lv[top].h + kPyrTY - 1) / kPyrTY;
    std::vector<PyrTile> tiles((size_t)ntx * nty);
    int bufMax = 0, tabMax = 0, dimMax = 0, winRows = 0, winCols = 0;
    auto up4 = [](int x) { return (x + 3) & ~3; };
    for (int ty = 0; ty < nty; ty++)
        for (int tx = 0; tx < ntx; tx++) {
            PyrTile &T = tiles[(size_t)ty * ntx + tx];
            std::memset(&T, 0, sizeof T);
            int x0 = 0, x1 = 0, y0 = 0, y1 = 0, tab = 0;
            for (int l = top; l >= 0; l--) {
                const DevLevel &D = P.lv[l];
                // own share of level l
                int ox0 = (int)((long long)D.w * tx / ntx), ox1 = (int)((long long)D.w * (tx + 1) / ntx);
                int oy0 = (int)((long long)D.h * ty / nty), oy1 = (int)((long long)D.h * (ty + 1) / nty);
                if (l < top) {
                    // what level l + 1's region [x0, x1) x [y0, y1) reads of level l
                    const DevLevel &U = P.lv[l + 1];
                    const int16_t *xofs = coef.data() + U.coefX;
                    const int nx0 = xofs[x0], nx1 = std::min(D.w, (int)xofs[x1 - 1] + 2);
                    const int ny0 = rowTab[(size_t)U.rowTab + y0].r0, ny1 = rowTab[(size_t)U.rowTab + y1 - 1].r1 + 1;
                    if (l == 0) { ox0 = nx0; ox1 = nx1; oy0 = ny0; oy1 = ny1; }          // level 0 is only read
                    else { ox0 = std::min(ox0, nx0); ox1 = std::max(ox1, nx1); oy0 = std::min(oy0, ny0); oy1 = std::max(oy1, ny1); }
                }
                if (l > 0) { x0 = ox0 & ~3; x1 = up4(ox1); } else { x0 = ox0 & ~3; x1 = ox1; }    // (level 0: dword loads from an aligned column)
                y0 = oy0; y1 = oy1;
                T.x0[l] = (int16_t)x0; T.x1[l] = (int16_t)x1; T.y0[l] = (int16_t)y0; T.y1[l] = (int16_t)y1;
                bufMax = std::max(bufMax, up4(x1 - x0) * (y1 - y0));
                if (l > 0) tab += (x1 - x0) + (y1 - y0);            // the tile's slices of the column and row tables (8 bytes an entry)
                if (l > 0) dimMax = std::max(dimMax, std::max(x1 - x0, y1 - y0));
                if (l == 0) { winRows = std::max(winRows, y1 - y0); winCols = std::max(winCols, x1 - x0); }
            }
            tabMax = std::max(tabMax, tab);
        }
    bufMax = (bufMax + 15) & ~15;
    if (2 * bufMax + 8 * tabMax <= 60 * 1024 && tiles.size() <= 4096 && P.nlevels <= 8 && dimMax <= 256 && winRows <= 80 && winCols <= 256) {   // (the kernel's fixed shapes: orb_pyramid.inc)
        if (h->dPyrTiles) { (void)hipFree(h->dPyrTiles); h->dPyrTiles = nullptr; }
        HIP_TRY(hipMalloc((void **)&h->dPyrTiles, tiles.size() * sizeof(PyrTile)));
        HIP_TRY(hipMemcpy(h->dPyrTiles, tiles.data(), tiles.size() * sizeof(PyrTile), hipMemcpyHostToDevice));
        h->nPyrTiles = (int)tiles.size(); h->pyrBuf = bufMax; h->pyrTab = tabMax;
    }
    return RUMI_OK;
}

static int set_geometry(RumiOrb *h, int w, int hgt) {
    if (h->gw == w && h->gh == hgt) return RUMI_OK;
    std::vector<LevelGeom> g;
    long long arena; int cells, cand, cellCand;
    if (!make_geometry(h->tab, w, hgt, g, &arena, &cells, &cand, &cellCand)) {
        g_lastError = "image too small for the FAST cell grid at some pyramid level, or cell larger than the LDS tile";
        return RUMI_E_INVALID;
    }
    if (arena > h->capArena || cells > h->capCells || cand > h->capCand || cellCand > h->capCellCand) {
        g_lastError = "image larger than the handle's max_width x max_height arenas";
        return RUMI_E_CAPACITY;
    }
    DevParams &P = h->hP;
    std::memset(&P, 0, sizeof P);
    P.nlevels = h->tab.nlevels; P.totalCells = cells; P.maxCellCand = h->capCellCand; P.totalCand = h->capCand;
    P.iniTh = std::min(std::max(h->cfg.ini_th_fast, 0), 255);   // cv::FAST clamps its threshold
    P.minTh = std::min(std::max(h->cfg.min_th_fast, 0), 255);
    P.arenaStride = h->capArena;
    for (int i = 0; i < 16; i++) P.umax[i] = h->tab.umax[i];
    std::vector<int16_t> coef;
    std::vector<RowTap> rowTab;
    make_level_tables(g, P, coef, rowTab);
    if ((int)coef.size() > h->capCoef) { g_lastError = "resize table capacity"; return RUMI_E_CAPACITY; }
    std::vector<uint16_t> octBins;
    make_octree_tables(P, octBins);
    if ((int)octBins.size() > h->capOctBins) { g_lastError = "quadtree coordinate table capacity"; return RUMI_E_CAPACITY; }
    // no room for this geometry's cell tables in the handle's arrays, or for k_compact's count table in LDS: its batches keep the one-launch quadtree
    if (P.octCellStride > h->capOctCells || oct_hist_lds_bytes(P.totalCells, P.octCellStride) == 0) P.octCellStride = 0;
    if (!octBins.empty()) HIP_TRY(hipMemcpy(h->dOctBins, octBins.data(), octBins.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->dP, &P, sizeof P, hipMemcpyHostToDevice));
    if ((int)rowTab.size() > h->capRowTab) { g_lastError = "resize row table capacity"; return RUMI_E_CAPACITY; }
    if (!coef.empty()) HIP_TRY(hipMemcpy(h->dCoef, coef.data(), coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    if (!rowTab.empty()) HIP_TRY(hipMemcpy(h->dRowTab, rowTab.data(), rowTab.size() * sizeof(RowTap), hipMemcpyHostToDevice));
    if (const int rcT = build_pyramid_tiles(h, coef, rowTab); rcT != RUMI_OK) return rcT;
    h->octLds = octree_lds_for(P, h->selLevelCap);
    if (h->octLds.wide > 160 * 1024) { g_lastError = "nfeatures too large for the LDS-resident quadtree node pool"; return RUMI_E_INVALID; }
    h->gw = w; h->gh = hgt;
    return RUMI_OK;
}

extern "C" int rumi_orb_tables(const RumiOrbConfig *cfg, float *scale, float *inv_scale, float *sigma2,
                               float *inv_sigma2, int32_t *features_per_level, int32_t *umax16) {
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels) return RUMI_E_INVALID;
    OrbTables t = make_tables(cfg->nfeatures, cfg->scale_factor, cfg->nlevels);
    for (int i = 0; i < t.nlevels; i++) {
        if (scale) scale[i] = t.scale[i];
        if (inv_scale) inv_scale[i] = t.invScale[i];
        if (sigma2) sigma2[i] = t.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = t.invSigma2[i];
        if (features_per_level) features_per_level[i] = t.featuresPerLevel[i];
    }
    if (umax16) for (int i = 0; i < 16; i++) umax16[i] = t.umax[i];
    return RUMI_OK;
}
