// The body of the one-wave-per-tile packet kernels (rts_kernels.hip): included by shadowMaskPacketKernel (LIVES false, ACTIVE false),
// by shadowMaskFollowKernel (LIVES true) and by shadowMaskActivePacketKernel (ACTIVE true), which name the template parameters
// K ... SEG, LIVES and ACTIVE and their kernel argument `p`.
// One text, three kernel templates: the code objects of shadowMaskPacketKernel are exactly those it had before follow mode and
// before active maps.
    static_assert(!ACTIVE || (K == 1 && WPB == 1 && !TILESPLIT && !LIVES), "an active map: the one-tile forms without a table only");
    static_assert(!BANDS || (PLAIN && K == 1 && WPB == 1), "the band form exists for the one-tile everyday launch only");
    static_assert(SPLIT == 1 || (K == 1 && WPB == 1 && SOFT), "samples are split over waves in the one-tile soft-shadow form only");
    static_assert(!TILESPLIT || (PLAIN && K == 1 && WPB == 1 && !SOFT && SPLIT == 1), "split tiles exist for the one-tile everyday launch only");
    static_assert(!SEG || WIDE == 1 || WIDE == 3, "the segment-ray forms exist in the assembly wide loop and the lane walk only");
    static_assert(!ALLTABLE || (TILESPLIT && !PIECES && !BANDS && WIDE == 1 && !LIVES), "ALLTABLE: a whole-dispatch table of the wide kernel, whole frames");
    __shared__ uint32_t shareSlots[WPB * SPLIT][64];     // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    // per-lane stacks of the wide lane walk: 4 KB per wave -- which caps a CU at 28 one-wave workgroups instead of 32, so
    // only the instantiations that use them (WIDE == 3: option "wide_lane") allocate them
    constexpr bool LANE_STACKS = WIDE == 3;
    __shared__ uint32_t laneStacks[LANE_STACKS ? WPB * SPLIT : 1][LANE_STACKS ? LANE_STACK * 64 : 1];
    uint32_t* laneStack = LANE_STACKS ? laneStacks[threadIdx.x >> 6] : nullptr;
    __shared__ uint32_t partial[SPLIT > 1 ? SPLIT : 1][SPLIT > 1 ? 64 : 1];                          // per-wave counts of unoccluded samples
    constexpr uint32_t TW = K >= 2 ? 16u : 8u, TH = K >= 4 ? 16u : 8u;
    uint32_t bx = blockIdx.x, by = 0;
    bool mine = true;
    if constexpr (ALLTABLE) {
        // The table holds every tile and nothing else (rts_alltable.h: allTableRule), so the wave is its record: no tile rows, no
        // bitmap, no piece path, no test against the record count.  What the record's address and the texel's need -- and the
        // address of the per-scene constants -- is asked for in ONE batch; then the record and the constants in a second.
        const uint64_t posAddr = (uint64_t)(uintptr_t)p.positions, frontAddr = (uint64_t)(uintptr_t)p.frontMap,
                       sceneAddr = (uint64_t)(uintptr_t)p.sceneBounds;
        const uint32_t a0 = p.W, a1 = p.rowBegin, a2 = p.rowEnd, a3 = p.blocksX, a4 = p.frontStride;
        asm volatile("" :: "s"(posAddr), "s"(frontAddr), "s"(sceneAddr), "s"(a0), "s"(a1), "s"(a2), "s"(a3), "s"(a4));
        const uint32_t id = blockIdx.y * a3 + blockIdx.x;             // (the grid is blocksX wide)
        const uint32_t slot = (id & 7u) * a4 + (id >> 3);             // (this XCD's run of the map: TraceParams::frontMap)
        const uint32_t tile = *(ConstU32Ptr)(uintptr_t)(frontAddr + (uint64_t)slot * 4u);
        bx = tile & 0xFFFFu; by = tile >> 16;
    } else if constexpr (PLAIN) {
        // Everything a tile wave needs before it can ask for its texel is the first 64 bytes of the argument block: asked for
        // here in one batch (the compiler would fetch each field where it is first used: three or four dependent round
        // trips to the scalar cache in front of the texel request).
        const uint64_t posAddr = (uint64_t)(uintptr_t)p.positions, mapAddr = (uint64_t)(uintptr_t)p.skipMap;
        const uint32_t a0 = p.W, a1 = p.rowBegin, a2 = p.rowEnd, a3 = p.pieceRows, a4 = p.blocksX, a5 = p.blocksY, a6 = p.rowOrder,
                       a7 = p.bandShift, a8 = p.stripe;
        asm volatile("" :: "s"(posAddr), "s"(mapAddr), "s"(a0), "s"(a1), "s"(a2), "s"(a3), "s"(a4), "s"(a5), "s"(a6), "s"(a7), "s"(a8));
        if constexpr (ACTIVE) {                                       // ... and the active map's address, in the same batch
            const uint64_t actAddr = (uint64_t)(uintptr_t)p.activeMap;
            asm volatile("" :: "s"(actAddr));
        }
    }
    if constexpr (ALLTABLE) {
    } else if constexpr (TILESPLIT) {
        const uint32_t pieceRows = p.pieceRows, blocksX = p.blocksX, blocksY = p.blocksY, rowOrder = p.rowOrder;
        const uint64_t mapAddr = uniform64(p.skipMap);
        if (blockIdx.y < pieceRows) {                                 // the head of the grid: records of the split table
            const uint32_t id = blockIdx.y * gridDim.x + blockIdx.x;
            if (id >= p.nPieces) return;
            const uint64_t mapFront = uniform64(p.frontMap);
            const uint32_t slot = (id & 7u) * p.frontStride + (id >> 3);       // (this XCD's run of the map: TraceParams::frontMap)
            const uint32_t tile = mapFront ? *(ConstU32Ptr)(uintptr_t)(mapFront + (uint64_t)slot * 4u) : 0xFFFFFFFFu;
            if (tile == 0xFFFFFFFFu) { if constexpr (PIECES) runPiece<BANDS>(p, lds); return; }   // a piece of a split tile: a path of its own
            bx = tile & 0xFFFFu; by = tile >> 16;                     // a FRONT tile: a long tile's own wave, started first
        } else {
            const uint32_t k = blockIdx.y - pieceRows;
            by = rowOrder == 1u ? blocksY - 1u - k : (rowOrder == 2u ? ((k & 1u) ? (blocksY >> 1) - ((k + 1u) >> 1) : (blocksY >> 1) + (k >> 1)) : k);
            // the tile's bit of the split table (the word travels with the next batch of kernel arguments)
            const uint32_t bit = by * blocksX + bx;
            const uint32_t word = *(ConstU32Ptr)(uintptr_t)(mapAddr + (uint64_t)(bit >> 5) * 4u);
            mine = !((word >> (bit & 31u)) & 1u);                    // a tile of the table is walked by its record(s) at the head
            if (!mine) return;                                       // (a scalar branch: nothing of this wave is needed)
        }
    } else by = dispatchRow(p, blockIdx.y);                           // (PLAIN: a 2-D grid, rows in dispatchRow order)
    if (!PLAIN && !blockToXY(p, blockIdx.x, &bx, &by)) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x0 = WPB == 4 ? bx * (2u * TW) + (wave & 1u) * TW + (lane & 7u) : bx * TW + (lane & 7u);     // (SPLIT: every wave, the same tile)
    const uint32_t v0 = (WPB == 4 ? by * (2u * TH) + (wave >> 1) * TH : by * TH) + (lane >> 3);
    bool live[K];
    size_t pix[K];
    F3 rel[K];
    [[maybe_unused]] uint8_t act = 0;                                 // ACTIVE: the pixel's byte of the active map
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t x = x0 + (k & 1) * 8u;
        uint32_t y;
        if constexpr (BANDS) {
            const uint32_t band = by >> p.bandShift, within = by - (band << p.bandShift);
            y = (band * p.nStripes + p.stripe) * p.bandRows + within * 8u + (lane >> 3);
        } else y = PLAIN ? p.rowBegin + v0 + (k >> 1) * 8u : ownedRow(p, v0 + (k >> 1) * 8u);
        live[k] = (x < p.W) && (y < p.rowEnd) && mine;
        pix[k] = (size_t)y * p.W + x;
        if constexpr (PLAIN) {
            // (no branch around the request: a lane without a pixel asks for texel 0 and never looks at it -- with the branch
            //  the compiler waits for the texel inside it, before the rest of the prologue's scalar work)
            const f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + (live[k] ? pix[k] : (size_t)0));   // comp:135
            // (ACTIVE: the byte is requested with the texel -- one batch, one wait -- and a lane without a pixel asks for byte 0)
            if constexpr (ACTIVE) act = __builtin_nontemporal_load(p.activeMap + (live[k] ? pix[k] : (size_t)0));
            rel[k] = F3{ t.x, t.y, t.z };
        } else {
            rel[k] = F3{ 0.f, 0.f, 0.f };
            if (live[k]) {
                f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + pix[k]);   // comp:135
                if constexpr (ACTIVE) act = __builtin_nontemporal_load(p.activeMap + pix[k]);
                rel[k] = F3{ t.x, t.y, t.z };
            }
        }
    }
    // ACTIVE: a lane walks when it owns a pixel AND the pixel's byte is set; it stores when it owns a pixel (0 where the byte is 0).
    [[maybe_unused]] bool owns = false;
    [[maybe_unused]] uint32_t rayPix = 0;
    if constexpr (ACTIVE) {
        owns = live[0];
        live[0] = owns && act != 0;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(live[0]);
        // A tile without a ray: one ballot, one scalar branch, the zero stores, end -- before the stream is opened or a ray is set
        // up.  (SPLIT: the four waves of the workgroup look at the same tile, so all of them leave here, in front of the barrier,
        // or none does.)
        if (walkers == 0) {
            if (owns && (SPLIT == 1 || wave == 0)) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix[0]]);
            return;
        }
        // Lanes that do not walk take the texel (and pixel index) of the first lane that does.  The ray set-up decides per WAVE
        // between forms that give the same bits wherever both apply (makeShadowRay's one-gate fast path, the rcpFast range
        // tests: ballots over all 64 lanes), so what such a lane holds can never change a walking lane's bits -- but a background
        // texel (0,0,0,0) or garbage (NaN, Inf, 1e38: allowed in an inactive pixel) would send the whole wave down the general
        // path.  With the stand-in every lane that does not walk sets up the very ray of a lane that does: it passes every gate
        // that lane passes.  Exact, because the stand-in only feeds lanes whose result is discarded (they are no members of the
        // walk, and the store below writes 0 for them).
        const int firstWalker = __builtin_ctzll(walkers);
        const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel[0].x), firstWalker));
        const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel[0].y), firstWalker));
        const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel[0].z), firstWalker));
        rel[0] = live[0] ? rel[0] : F3{ sx, sy, sz };
        if constexpr (SOFT) {                                         // (the pixel index picks the light sample: per-pixel jitter)
            const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pix[0], firstWalker);
            rayPix = live[0] ? (uint32_t)pix[0] : sp;
        }
    }
    const NodeStream bvh = openStream(p);
    const uint32_t ns = SOFT ? p.nsamples : 1u;
    // clock probe (every instantiation, so that the clock is measured on the launches that are timed): one wave per tile row
    // (the stamps go straight to memory: nothing of the probe stays in registers across the walk)
    // (with a table: the tile rows stamp; when the table holds every tile there are none, and the front-tile rows stamp instead)
    const uint32_t probeRow = ALLTABLE ? blockIdx.y : TILESPLIT ? (p.allInTable ? blockIdx.y : blockIdx.y - p.pieceRows) : (p.grid2d ? blockIdx.y : 0u);
    const bool probed = p.clockProbe != nullptr && blockIdx.x == 0 && threadIdx.x == 0 &&
                        (ALLTABLE ? blockIdx.y < p.blocksY : (!TILESPLIT || (p.allInTable ? blockIdx.y < p.blocksY : blockIdx.y >= p.pieceRows)));
    if (probed) {
        uint64_t* o = p.clockProbe + (size_t)probeRow * 4;
        o[0] = __builtin_amdgcn_s_memtime(); o[2] = __builtin_amdgcn_s_memrealtime();
    }
    if constexpr (LIVES) {              // follow mode: the wave's start, one vector store by lane 0 (tile id = row-major in the dispatch)
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
        if (lane == 0) p.followLives[(size_t)(by * p.blocksX + bx) * 2u] = t0;
        __builtin_amdgcn_s_waitcnt(0xC07F);     // (lgkmcnt(0) alone: the stamp's wait is not left to the walk's first LDS waits)
    }
    const uint64_t tStart = !PLAIN && p.waveStats ? __builtin_amdgcn_s_memtime() : 0;   // diagnostics only
    const uint64_t rStart = !PLAIN && p.waveStats ? __builtin_amdgcn_s_memrealtime() : 0;
    int32_t left = 0;
    ShareDiag shareDiag;
    shareDiag.on = !PLAIN && p.waveStats != nullptr;
    uint32_t lit[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lit[k] = 0;
    uint64_t tReady = 0;
    for (uint32_t s = SPLIT > 1 ? wave : 0u; s < ns; s += SPLIT) {
        Ray r[K];
        bool occluded[K];
        [[maybe_unused]] bool fast = false;
        [[maybe_unused]] float sceneRoot[6];
        if constexpr (ALLTABLE) {
            // the root box and wideSetupBound of it: computed when the stream's boxes change (sceneBoundsKernel), not per wave
            const uint64_t sceneAddr = (uint64_t)(uintptr_t)p.sceneBounds;
            const u32x8 c = *(ConstNodePtr)(uintptr_t)sceneAddr;
            const uint32_t bz = *(ConstU32Ptr)(uintptr_t)(sceneAddr + 32u);
            sceneRoot[0] = __uint_as_float(c.s0); sceneRoot[1] = __uint_as_float(c.s1); sceneRoot[2] = __uint_as_float(c.s2);
            sceneRoot[3] = __uint_as_float(c.s4); sceneRoot[4] = __uint_as_float(c.s5); sceneRoot[5] = __uint_as_float(c.s6);
            r[0] = makeShadowRay<true>(p, rel[0], s, (uint32_t)pix[0], &fast, SetupBound{ c.s3, c.s7, bz });
        } else if constexpr (WIDE != 0) {
            float rootLo[3], rootHi[3];
            wideRoot(p, rootLo, rootHi);
            r[0] = makeShadowRay<!SOFT && WIDE != 3>(p, rel[0], s, ACTIVE ? rayPix : (uint32_t)pix[0], &fast, wideSetupBound(rootLo, rootHi));
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = makeShadowRay<!SOFT>(p, rel[k], s, ACTIVE ? rayPix : (uint32_t)pix[k]);
        }
        if (!PLAIN && p.waveStats && s < SPLIT) {    // diagnostics: the G-buffer texel is in and the first ray exists
            asm volatile("" :: "v"(r[0].inv.x), "v"(r[0].inv.y), "v"(r[0].inv.z), "v"(r[0].o.x));
            tReady = __builtin_amdgcn_s_memtime();
        }
        if constexpr (ALLTABLE) occluded[0] = traverseWideScene<SEG>(p, sceneRoot, sceneRoot + 3, r[0], live[0], lds, laneStack, &left, &shareDiag, fast);
        else if constexpr (WIDE != 0) occluded[0] = traverseWide<WIDE != 2, SEG>(p, bvh, r[0], live[0], lds, laneStack, &left, &shareDiag, fast);
        else traversePacket<K, PREFETCH>(p, bvh, r, live, occluded, lds, &left, &shareDiag);
#pragma unroll
        for (int k = 0; k < K; ++k) lit[k] += occluded[k] ? 0u : 1u;                     // comp:148
    }
    // (8-byte row stores built from a ballot were tried: WRITE_SIZE stayed at 40 MB per 8.3 MB mask -- the
    // memory side counts 32-byte sectors either way -- and the kernel got 10 % slower; byte stores stay.)
    if constexpr (SPLIT > 1) {
        partial[wave][lane] = lit[0];
        __syncthreads();
        if (wave == 0) {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < SPLIT; ++w) sum += partial[w][lane];
            if constexpr (ACTIVE) { if (owns) __builtin_nontemporal_store((uint8_t)(live[0] ? sum : 0u), &p.mask[pix[0]]); }
            else if (live[0]) __builtin_nontemporal_store((uint8_t)sum, &p.mask[pix[0]]);     // comp:150
        }
    } else if constexpr (ACTIVE) {
        if (owns) __builtin_nontemporal_store((uint8_t)(live[0] ? lit[0] : 0u), &p.mask[pix[0]]);   // comp:150; 0 = no ray was sent
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
#ifdef RTS_EXPERIMENT_NO_MASK_STORE      // (experiment build only, tools/mask_store_ab.sh: what the byte stores cost -- nothing is ever stored)
            if (live[k] && lit[k] > 200u) __builtin_nontemporal_store((uint8_t)lit[k], &p.mask[pix[k]]);
#else
            if (live[k]) __builtin_nontemporal_store((uint8_t)lit[k], &p.mask[pix[k]]);   // comp:150
#endif
    }
    if constexpr (LIVES) {              // ... and its end, after the mask bytes are stored
        const uint32_t t1 = (uint32_t)__builtin_amdgcn_s_memrealtime();
        if (lane == 0) p.followLives[(size_t)(by * p.blocksX + bx) * 2u + 1u] = t1;
    }
    if (probed) {
        uint64_t* o = p.clockProbe + (size_t)probeRow * 4;
        uint32_t hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        // (the wave's hardware slot rides in the top 16 bits of the end stamp: 2^48 shader clocks are 32 hours)
        o[1] = (__builtin_amdgcn_s_memtime() & 0x0000FFFFFFFFFFFFull) | ((uint64_t)(hwid & 0xFFFFu) << 48);
        o[3] = __builtin_amdgcn_s_memrealtime();
    }
    if (!PLAIN && p.waveStats && lane == 0) {    // diagnostics: never read by any kernel, never part of an output
        const size_t slot = (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (WPB * SPLIT) + wave;
        uint64_t* o = p.waveStats + slot * 4;
        o[0] = tStart;
        o[1] = __builtin_amdgcn_s_memtime();
        // shader clocks against the 100 MHz reference over the same interval: the clock the chip held under this load
        p.waveRealtime[slot * 4] = rStart;
        p.waveRealtime[slot * 4 + 1] = __builtin_amdgcn_s_memrealtime();
        p.waveRealtime[slot * 4 + 2] = tReady - tStart;      // clocks from wave start to "first ray ready"
        uint32_t xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));       // wave slot, SIMD, CU, SE ... of this wave
        p.waveRealtime[slot * 4 + 3] = ((uint64_t)hwid << 32) | xcc;
        // dissolved flag | lane-per-ray iterations after the dissolve | clocks from start to the dissolve
        o[2] = (left < 0 ? 1ull : 0ull) | ((uint64_t)(shareDiag.iterations & 0xFFFFFFu) << 8) |
               ((shareDiag.tDissolve ? (shareDiag.tDissolve - tStart) & 0xFFFFFFFFull : 0ull) << 32);
        o[3] = ((uint64_t)bx << 48) | ((uint64_t)(by & 0xFFFFu) << 32) | shareDiag.laneSteps;   // ... and the lane-steps in them
    }
