// trc_stream.inc -- streaming ("wavefront") form of the fast engine.  Included by trc_kernels.hip.
//
// The persistent megakernel (k_trace_coop) keeps a ray in registers through generation, search, exact tests and
// shading; that makes it a fat kernel (256 VGPRs, 2 waves per SIMD) whose phases run at 12-50 % lane utilisation,
// while HBM sits idle (0.9 GB of traffic in a 27 ms launch).  Here the phases are separate, lean kernels connected
// by queues in HBM, so that each one runs with (nearly) every lane busy and many waves per SIMD:
//
//   k_s_gen    generate (or load) rays, float64 entry into the scene box, quick reject; rays with candidates are written
//              to the ray table and, if they enter the box of the search structure, appended to the walker queue Q1
//              (single-precision ray, interval); surfaces tested for every ray (those set apart from the grid, the
//              Kd-tree's always-relevant ones, unbounded ones) go straight to the candidate queue Q3
//   k_s_walk   single precision only: each lane steps through the uniform grid (or walks the Kd-tree) for one Q1 entry
//              and lists the non-empty cells / leaves it crosses; the wave drains the lists together (balanced box
//              tests) and appends (ray, surface) survivors to Q3
//   k_s_exact  one lane per Q3 entry: exact float64 trc_intersect; an entry with a finite t links itself into its ray's
//              list of hits (one atomicExch on the ray record), the first one also appends the ray to the hit list
//   k_s_shade  one lane per hit ray: walks the ray's (1-3) linked hits for the nearest one, lowest surface index on equal
//              t (the reference's tie rule); normal, optics, tallies (LDS-privatised), flux map, hit capture; the continued ray is
//              written back to the table and appended to the next bounce's active list
//
// What k_s_fresh, k_s_fresh2 and k_s_bounce share is written once, in trc_device.h: the LDS image of their tables
// (trc_search_lds_layout, trc_bounds.h: the kernels carve their pointers from it, the host sizes the launches and decides "fits in
// LDS" from the same function) and its staging (stage_search_tables), the search of a listed fresh ray (listed_ray_search), the
// Buie table's fill (buie_tables_fill), a fresh ray's record and a hit-list entry (store_fresh_ray, store_hit).  k_s_gen and
// k_s_bounce_coop keep their own copies: through the helpers their instances changed registers or scratch.
//
// Results are those of the other engines ray for ray: the same per-ray functions of trc_core.h, the same Philox
// streams (stream id = ray_offset + index in the call), the same candidates, the same tie rule.


template <bool FRESH, int KIND>
__device__ __forceinline__ void s_gen_body(const StreamParams &S, trc_buie_fast &l_bf) {
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const bool buie_src = FRESH && P.src && (P.src->kind == TRC_SRC_BUIE_DISK || P.src->kind == TRC_SRC_BUIE_RECT);
    if (buie_src) trc_buie_fast_fill(P.src->buie, &l_bf, 0, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    if (buie_src) trc_buie_fast_fill(P.src->buie, &l_bf, 1, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    const trc_accel_view A = stream_accel_global(sc, S.search);
    // FRESH: the rays of the batch, or those k_s_fresh left to this path (their numbers in gen_list); else the active list
    const uint32_t *list = FRESH ? S.gen_list : S.act_in;
    long long count = FRESH ? (list ? (long long)W.cnt[CN(CW_GEN_LIST)] : S.nb) : (long long)W.cnt[CN(CW_ACT_IN)];
    if (list && count > (FRESH ? SQ_ROOM(W) : W.act_room)) count = FRESH ? SQ_ROOM(W) : W.act_room;
    const long long padded = (count + 63) & ~63ll;
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk c1 = S.static_general ? chunk_init_static(S.chunk_q1, wave_g) : chunk_init(S.chunk_q1);
    // re-entering rays mostly have a candidate among the surfaces set apart (they were aimed at one): pre-assigned too
    WaveChunk c3 = (!FRESH && S.q3_gen_chunk0 >= 0) ? chunk_init_static(S.chunk_q3, (unsigned long long)S.q3_gen_chunk0 + wave_g) : chunk_init(S.chunk_q3);
    WaveChunk cs = (FRESH && S.static_general) ? chunk_init_static_at(SQ_CHUNK, (unsigned long long)S.slot_base0 + wave_g * SQ_CHUNK) : chunk_init();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += (long long)gridDim.x * blockDim.x) {
        bool valid = i < count;
        uint32_t slot = 0, ri = 0;
        double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 1, e = 0, ref = 1.0, wl = 0.0;
        unsigned long long rid;
        if (valid) {
            if (FRESH) {
                ri = list ? list[i] : (uint32_t)i;
                if (ri == SQ_INVALID) { valid = false; ri = 0; }
                else fast_new_ray<KIND>(P, nullptr, S.base + ri, px, py, pz, dx, dy, dz, e, ref, wl, rid, buie_src ? &l_bf : nullptr);
            } else {
                slot = S.act_in[i];
                if (slot == SQ_INVALID) { valid = false; slot = 0; }
                else {
                    const SRayGeo g = W.geo[slot];
                    px = g.px; py = g.py; pz = g.pz; dx = g.dx; dy = g.dy; dz = g.dz;
                }
            }
        }
        if (!__ballot(valid)) continue;       // the unused tail of a chunk of the list: nothing to do, nothing to append
        trc_ray32 r;
        double t0;
        bool in = trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0);
        float tmin = 1.0f, tmax = 0.0f;
        bool walking = false;
        unsigned alw_mask = 0;
        bool cand = false;
        if (valid && in) {
            walking = trc_kd32_root(A.root, r, &tmin, &tmax);
            for (int k = 0; k < A.n_always; ++k) {
                const float *b = A.sbox + 6 * (size_t)A.always[k];
                bool bounded = !(b[3] == TRC_INF && b[0] == -TRC_INF);
                if (bounded && (k >= 32 || trc_box_hit32(b, r))) { if (k < 32) alw_mask |= 1u << k; cand = true; }
            }
            cand = cand || walking;
        }
        cand = valid && (cand || A.n_unbounded > 0);
        if (FRESH) {                    // a ray with a candidate takes the next slot of the table
            const unsigned long long sl = chunk_append(&W.cnt[CN(CW_SLOTS)], cs, cand, nullptr, 0);
            if (cand) {
                if ((long long)sl < SQ_ROOM(W)) slot = (uint32_t)sl;
                else { W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; cand = false; }
            }
        }
        if (cand) {
            if (FRESH) {                // a continued ray was written back by k_s_shade, search fields reset
                SRayGeo g;
                g.px = px; g.py = py; g.pz = pz; g.dx = dx; g.dy = dy; g.dz = dz;
                g.head = SQ_INVALID;
                g.idx = ri;
                g.tail = sray_tail(0, 0u);
                W.geo[slot] = g;
            }
            if (FRESH && !P.src) {      // rays of a source descriptor all carry (energy, 1, 0): written on their first hit only
                SRayAux a;
                a.e = e; a.ref = ref; a.wl = wl; a.pad = 0.0;
                W.aux[slot] = a;
            }
        }
        // rays that enter the root box go to the walker queue Q1
        const bool towalk = cand && walking;
        unsigned long long q = chunk_append(&W.cnt[CN(CW_Q1)], c1, towalk, W.q1_slot, SQ_ROOM(W));
        if (towalk) {
            if ((long long)q < SQ_ROOM(W)) {
                W.q1_slot[q] = slot;
                W.q1_a[q] = make_float4(r.ox, r.oy, r.oz, r.ix);
                W.q1_b[q] = make_float4(r.iy, r.iz, tmin, tmax);
            } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
        }
        // surfaces without bounds (infinite planes, cylinders ...): every ray is a candidate
        for (int k = 0; k < A.n_unbounded; ++k) {
            unsigned long long q3 = chunk_append(&W.cnt[CN(CW_Q3)], c3, cand, W.q3_slot, W.q3_cap);
            if (cand) {
                if ((long long)q3 < W.q3_cap) { W.q3_slot[q3] = slot; W.q3_surf[q3] = (uint32_t)A.unbounded[k]; }
                else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_RETRY;
            }
        }
        // always-relevant surfaces whose box the ray crosses: straight to the exact queue
        for (int k = 0; k < A.n_always; ++k) {
            bool want = cand && in && (k < 32 ? ((alw_mask >> k) & 1u) != 0 : true);
            if (k >= 32 && want) {
                const float *b = A.sbox + 6 * (size_t)A.always[k];
                want = !(b[3] == TRC_INF && b[0] == -TRC_INF) && trc_box_hit32(b, r);
            }
            if (want) want = trc_obb_hit32(sc.a_obb + (size_t)TRC_OBB_STRIDE * (size_t)A.always[k], r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
            unsigned long long q3 = chunk_append(&W.cnt[CN(CW_Q3)], c3, want, W.q3_slot, W.q3_cap);
            if (want) {
                if ((long long)q3 < W.q3_cap) { W.q3_slot[q3] = slot; W.q3_surf[q3] = (uint32_t)A.always[k]; }
                else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_RETRY;
            }
        }
    }
    chunk_close(c1, W.q1_slot, SQ_ROOM(W));
    chunk_close(c3, W.q3_slot, W.q3_cap);
}

// generic instance: any source kind (or given rays, or re-entering rays)
template <bool FRESH, int KIND = -1>
__global__ __launch_bounds__(256) void k_s_gen(StreamParams S) {
    __shared__ trc_buie_fast l_bf;
    s_gen_body<FRESH, KIND>(S, l_bf);
}

// an arc-lamp kind compiled in (trc_lamp_ray_t): k_s_gen<true, KIND>'s body under a name of its own, so that the family of k_s_gen
// stays the instances it was
template <int KIND>
__global__ __launch_bounds__(256) void k_s_gen_lamp(StreamParams S) {
    __shared__ trc_buie_fast l_bf;
    s_gen_body<true, KIND>(S, l_bf);
}

// the thermal emitter compiled in (trc_thermal_ray): k_s_gen<true, TRC_SRC_EMIT_THERMAL>'s body under a name of its own, as the lamps'
__global__ __launch_bounds__(256) void k_s_gen_emit(StreamParams S) {
    __shared__ trc_buie_fast l_bf;
    s_gen_body<true, TRC_SRC_EMIT_THERMAL>(S, l_bf);
}

// one source kind compiled in (Buie disc, pillbox disc / rectangle -- the Buie rectangle would spill): fits 128 registers, and
// four waves per SIMD instead of three are worth 6 % of the kernel
template <int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_s_gen_src(StreamParams S) {
    __shared__ trc_buie_fast l_bf;
    s_gen_body<true, KIND>(S, l_bf);
}

// ---------------------------------------------------------------------------------------------------------------
// Fresh rays of a plane source with a narrow cone (trc_footprint.h): bounce 0 in two kernels.
//   k_s_cull   every ray: its Philox block, the float32 start point on the source plane, one bit of the footprint mask (LDS).
//              A ray that starts outside every footprint cannot hit anything: it is finished here -- 81 % of the NSTTF rays,
//              before their direction is sampled.  Rays of the Buie aureole go to the general path (gen_list -> k_s_gen<true>
//              -> k_s_walk -> k_s_exact); the others are listed (ray number, mask cell) for k_s_fresh.  A lean kernel of its own:
//              a handful of arguments, ~40 registers, 8 waves per SIMD -- inside one kernel with the rest the round keys of
//              Philox lived in spilled scalar registers and the whole ran at 2 waves per SIMD;
//   k_s_ucull  the same decision without a start point, for the Buie sources in front of k_s_fresh2: the footprint mask tabulated
//              over the two position uniforms (umask, trc_footprint.h), indexed by the top bits of o[0] and o[1] -- a shift, an
//              alignbit and a bit-field extract, one LDS read, the bit test -- and the aureole by one unsigned compare of o[2]
//              with a threshold of the host's (trc_fp_generic_threshold).  No conversion, square root, sine, cosine, cell or
//              float64 compare: 72 vector instructions per ray instead of 104, 40 of them Philox (NSTTF: 0.159 -> 0.122 ms per 5e7
//              rays).  It lists the ray number alone (fq_cell is neither computed nor written); k_s_fresh2 derives the list cell
//              in its phase 1.  The mask in uniform space lists 2.7 % more NSTTF rays than the Cartesian one (19.6 % / 19.1 %);
//              lists, chunks and grids behind it are sized by its own share (ucoverage).  Both forms are one body
//              (s_cull_body<KIND, UM>); profiles/umask.txt says which instance uses which;
//   k_s_fresh  one lane per listed ray, every lane busy: the float64 ray exactly as k_s_gen makes it (trc_source_ray_t, same
//              stream), the surfaces listed for its cell, their oriented boxes in float32, the exact float64 test of those that
//              pass (the reference's tie rule: nearest, lowest surface index on equal t).  A ray that hits takes the next slot
//              of the ray table and goes straight to the hit list of k_s_shade, surface and distance with it.
// No ray record, walker or candidate entry is written for a ray that hits nothing.
// (SC_THREADS, SC_GEN_CAP, SF_THREADS and the other launch shapes: trc_forms.h, where the host sizes the launches)
struct CullParams {
    trc_fp_params F;
    const uint32_t *mask;
    unsigned long long seed, rid0;      // stream id of ray i of the batch: rid0 + i
    long long nb;
    uint32_t *fq_ray, *fq_cell;         // out: rays that may hit something
    uint32_t *gen_list;                 // out: rays of the general path
    unsigned long long *cnt;
    long long room;                     // entries in each of the lists
    unsigned chunk;                     // entries of fq reserved per atomic
    unsigned gen_chunk;                 // general-path list: entries pre-assigned per wave, or 0: the rays of a workgroup are
                                        // collected in LDS and appended with one atomic (they are rare: 4e-4 of the NSTTF rays; one
                                        // chunk per wave would leave k_s_gen a list of a few rays per 64 entries)
    int static_first;
    // the mask as the instance takes it: its words, and for the form over the uniforms (UM) its dimensions Mu = 1 << lu,
    // Mv = 1 << lv and trc_fp_generic as a compare of o[2] (trc_fp_generic_threshold)
    int mask_words;
    int lu, lv;
    int gen_on;
    uint32_t gen_thr;
};

template <int KIND, bool UM>
__device__ __forceinline__ void s_cull_body(const CullParams &C) {
    extern __shared__ double lds[];
    uint32_t *l_mask = (uint32_t *)lds;
    const trc_fp_params &F = C.F;
    uint32_t *l_gen = l_mask + C.mask_words;           // [SC_GEN_CAP] rays | count | base of the flush
    uint32_t *l_gen_n = l_gen + SC_GEN_CAP;
    for (int i = threadIdx.x; i < C.mask_words; i += SC_THREADS) l_mask[i] = C.mask[i];
    if (threadIdx.x == 0) { l_gen_n[0] = 0u; l_gen_n[1] = 0u; }
    __syncthreads();
    const unsigned lane = lane_id();
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * SC_THREADS + threadIdx.x) >> 6;
    const long long n_waves = (long long)gridDim.x * (SC_THREADS / 64);
    WaveChunk cf = C.static_first ? chunk_init_static(C.chunk, wave_g) : chunk_init(C.chunk);
    WaveChunk cg = (C.static_first && C.gen_chunk) ? chunk_init_static(C.gen_chunk, wave_g) : chunk_init(C.gen_chunk ? C.gen_chunk : 64u);
    const long long n_groups = (C.nb + 63) >> 6;
    for (long long g = (long long)wave_g; g < n_groups; g += n_waves) {
        const long long i = g * 64 + lane;
        const bool valid = i < C.nb;
        const unsigned long long rid = C.rid0 + (unsigned long long)i;
        uint32_t o[4];
        trc_philox4x32_10((uint32_t)rid, (uint32_t)(rid >> 32), 0u, 0u, (uint32_t)C.seed, (uint32_t)(C.seed >> 32), o);   // = trc_uniform_quad's block
        int32_t ix = 0, iy = 0;
        bool bit, generic;
        if constexpr (UM) {         // the position uniforms' top bits are the mask index: no start point
            constexpr int U = KIND == TRC_SRC_PILLBOX_DISK || KIND == TRC_SRC_PILLBOX_RECT ? 2 : 0;
            uint32_t word, b;
            trc_fp_ucell(o[U], o[U + 1], C.lu, C.lv, &word, &b);
            bit = ((l_mask[word] >> b) & 1u) != 0u;
            generic = valid && trc_fp_generic_u(C.gen_on != 0, C.gen_thr, o[2]);
        } else {
            float lx, ly;
            trc_fp_position32_t<KIND>(F, o, &lx, &ly);
            trc_fp_cell(F, lx, ly, &ix, &iy);
            bit = ((l_mask[((uint32_t)iy * (uint32_t)F.M + (uint32_t)ix) >> 5] >> (ix & 31)) & 1u) != 0u;
            generic = valid && trc_fp_generic(F, o);
        }
        if (C.gen_chunk) {
            const unsigned long long qg = chunk_append(&C.cnt[CN(CW_GEN_LIST)], cg, generic, C.gen_list, C.room);
            if (generic) { if ((long long)qg < C.room) C.gen_list[qg] = (uint32_t)i; else C.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; }
        } else if (generic) {
            const uint32_t at = atomicAdd(&l_gen_n[0], 1u);
            if (at < SC_GEN_CAP) l_gen[at] = (uint32_t)i;
            else {      // the workgroup's list is full (the source is not what the host took it for): one entry, one atomic
                const unsigned long long qg = atomicAdd(&C.cnt[CN(CW_GEN_LIST)], 1ull);
                if ((long long)qg < C.room) C.gen_list[qg] = (uint32_t)i; else C.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
            }
        }
        const bool pass = valid && !generic && bit;
        const unsigned long long q = chunk_append(&C.cnt[CN(CW_FP_LIST)], cf, pass, C.fq_ray, C.room);
        if (pass) {
            if ((long long)q < C.room) {
                C.fq_ray[q] = (uint32_t)i;
                if constexpr (!UM) C.fq_cell[q] = ((uint32_t)iy << 16) | (uint32_t)ix;
            } else C.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
        }
    }
    if (C.gen_chunk) chunk_close(cg, C.gen_list, C.room);
    chunk_close(cf, C.fq_ray, C.room);
    if (!C.gen_chunk) {
        __syncthreads();
        uint32_t n = l_gen_n[0];
        if (n > SC_GEN_CAP) n = SC_GEN_CAP;
        if (threadIdx.x == 0 && n) {
            const unsigned long long b = atomicAdd(&C.cnt[CN(CW_GEN_LIST)], (unsigned long long)n);
            l_gen_n[1] = (uint32_t)b;           // the list holds fewer than 2^32 entries (room <= 2^26 + slack)
            if ((long long)(b + n) > C.room) { C.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; l_gen_n[0] = 0u; }
        }
        __syncthreads();
        n = l_gen_n[0] > SC_GEN_CAP ? SC_GEN_CAP : l_gen_n[0];
        const uint32_t b = l_gen_n[1];
        for (uint32_t k = threadIdx.x; k < n; k += SC_THREADS) C.gen_list[(size_t)b + k] = l_gen[k];
    }
}
// the form on the Cartesian mask, which hands k_s_fresh the cell / the form on the mask over the uniforms, in front of k_s_fresh2
template <int KIND>
__global__ __launch_bounds__(SC_THREADS) void k_s_cull(CullParams C) { s_cull_body<KIND, false>(C); }
template <int KIND>
__global__ __launch_bounds__(SC_THREADS) void k_s_ucull(CullParams C) { s_cull_body<KIND, true>(C); }

#ifndef SB_FLAT_WALK
#define SB_FLAT_WALK 0          /* 1: the grid that fits LDS is walked like the large one, one cell or one candidate per lane and turn */
#endif

// FLAT: every surface of the scene is a flat kind (a heliostat field, a mesh): the instance carries no quadric code.
// LDS: the tables a listed ray reads (surface records, oriented boxes, cell lists) are staged in LDS -- all of them or none, so
// that the compiler knows the address space of every access (a pointer that may be either is read with flat loads).
// (their LDS image: fresh_lds_parts, trc_forms.h)

template <int KIND, bool FLAT, bool LDS>
__global__ __launch_bounds__(SF_THREADS(FLAT)) void k_s_fresh(StreamParams S) {
    constexpr int THREADS = SF_THREADS(FLAT);
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    constexpr bool BUIE = KIND == TRC_SRC_BUIE_DISK || KIND == TRC_SRC_BUIE_RECT;
    const trc_lds_parts parts = fresh_lds_parts(sc.n_surf, sc.stride, S.fp.P, S.fp.n_list, BUIE, LDS, 0);
    const trc_lds_layout L = trc_search_lds_layout(parts);
    trc_buie_fast *l_bf = BUIE ? (trc_buie_fast *)((char *)lds + L.buie) : nullptr;
    const double *recs = sc.recs;
    const float *obb = sc.a_obb;
    typedef fp_list_t<LDS> list_t;
    const list_t *l_coff = nullptr, *clist = (const list_t *)S.fp.clist;
    stage_search_tables<THREADS>((char *)lds, L, parts, sc, S.fp, (int)threadIdx.x);
    if (LDS) {
        recs = (const double *)((char *)lds + L.recs); obb = (const float *)((char *)lds + L.obb);
        l_coff = (const list_t *)((char *)lds + L.fp_off); clist = (const list_t *)((char *)lds + L.fp_list);
    }
    buie_tables_fill(P.src, l_bf, (int)threadIdx.x, (int)blockDim.x, BUIE);
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    long long count = (long long)W.cnt[CN(CW_FP_LIST)];
    if (count > SQ_ROOM(W)) count = SQ_ROOM(W);
    const long long padded = (count + 63) & ~63ll;
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * THREADS + threadIdx.x) >> 6;
    WaveChunk cs = S.static_first ? chunk_init_static(S.chunk_slot, wave_g) : chunk_init(S.chunk_slot);       // slots of the ray table
    WaveChunk ch = S.static_first ? chunk_init_static(S.chunk_hit, wave_g) : chunk_init(S.chunk_hit);         // hit list
    // the entry of the next iteration is fetched while this one is worked on (3 waves per SIMD do not hide an HBM round trip)
    uint32_t ri_n = SQ_INVALID, cell_n = 0;
    {
        const long long i0 = (long long)blockIdx.x * THREADS + threadIdx.x;
        if (i0 < count) { ri_n = W.fq_ray[i0]; cell_n = W.fq_cell[i0]; }
    }
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < padded; i += (long long)gridDim.x * THREADS) {
        const uint32_t ri = ri_n, cell = cell_n;
        {
            const long long i1 = i + (long long)gridDim.x * THREADS;
            ri_n = SQ_INVALID; cell_n = 0;
            if (i1 < count) { ri_n = W.fq_ray[i1]; cell_n = W.fq_cell[i1]; }
        }
        const bool active = ri != SQ_INVALID;
        if (!__ballot(active)) continue;
        listed_ray_search<KIND, FLAT, LDS>(S, l_bf, recs, obb, l_coff, clist, cs, ch, active, ri, cell);
    }
    chunk_close(ch, W.hit_slot, SQ_ROOM(W));
}

// The same in two phases, for the Buie sources (k_s_fresh2).  Two of three listed rays of the NSTTF field miss every surface listed
// for their cell: the list was made before their direction was known (a 4.65 mrad cone over 300 m is 1.4 m of margin around a 6 m
// mirror), and each of them pays the whole float64 sampling of the source -- 250 of the kernel's 545 vector instructions per ray --
// to fail an oriented box.  Phase 1, every listed ray: its Philox block, the start point in float32 as k_s_cull takes it, the
// direction in float32 (polar angle from the table, sine and cosine of a milliradian angle by two terms of their series), the
// oriented boxes of the cell's surfaces.  The float32 ray is within 1e-4 m of the float64 one on the mirrors; the boxes carry
// delta >= 1e-3 m (1e-2 on the NSTTF field) on every side, so a ray that hits a surface passes its box in this form too.  The
// rays that pass wait in a queue of the wave in LDS; whenever 64 of them have come together the wave runs phase 2 with every
// lane busy: the float64 ray, boxes and exact tests exactly as k_s_fresh does them.
template <int KIND, bool FLAT, bool LDS>
__global__ __launch_bounds__(SF_THREADS(FLAT)) void k_s_fresh2(StreamParams S0) {
    constexpr int THREADS = SF_THREADS(FLAT);
    extern __shared__ double lds[];
    // (one explicit argument: kernel_args_again.  The instances with their tables in LDS read it again in every turn of the loop;
    // those with the tables in global memory came out with more vector registers that way and keep the by-value block)
    const StreamParams &S = S0;
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const trc_fp_params &F = S.fp.P;
    static_assert(KIND == TRC_SRC_BUIE_DISK || KIND == TRC_SRC_BUIE_RECT, "the two-phase form samples the Buie direction in float32");
    const trc_lds_parts parts = fresh_lds_parts(sc.n_surf, sc.stride, S.fp.P, S.fp.n_list, true, LDS, THREADS / 64);
    const trc_lds_layout L = trc_search_lds_layout(parts);
    trc_buie_fast *l_bf = (trc_buie_fast *)((char *)lds + L.buie);
    const double *recs = sc.recs;
    const float *obb = sc.a_obb;
    typedef fp_list_t<LDS> list_t;
    const list_t *l_coff = nullptr, *clist = (const list_t *)S.fp.clist;
    stage_search_tables<THREADS>((char *)lds, L, parts, sc, S.fp, (int)threadIdx.x);
    if (LDS) {
        recs = (const double *)((char *)lds + L.recs); obb = (const float *)((char *)lds + L.obb);
        l_coff = (const list_t *)((char *)lds + L.fp_off); clist = (const list_t *)((char *)lds + L.fp_list);
    }
    // the queue of this wave: SFQ_CAP ray numbers, then their cells
    uint32_t *q_ray = (uint32_t *)((char *)lds + L.queues) + (size_t)(threadIdx.x >> 6) * (2 * SFQ_CAP);
    uint32_t *q_cell = q_ray + SFQ_CAP;
    buie_tables_fill(P.src, l_bf, (int)threadIdx.x, (int)blockDim.x, true);
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    long long count = (long long)W.cnt[CN(CW_FP_LIST)];
    if (count > SQ_ROOM(W)) count = SQ_ROOM(W);
    const long long padded = (count + 63) & ~63ll;
    const unsigned lane = lane_id();
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * THREADS + threadIdx.x) >> 6;
    WaveChunk cs = S.static_first ? chunk_init_static(S.chunk_slot, wave_g) : chunk_init(S.chunk_slot);       // slots of the ray table
    WaveChunk ch = S.static_first ? chunk_init_static(S.chunk_hit, wave_g) : chunk_init(S.chunk_hit);         // hit list
    // the source in float32: centre relative to the scene's, the two columns of the position frame, the direction frame
    const trc_source_desc *src = P.src;
    const float c0 = (float)(src->center[0] - sc.a_cen[0]), c1 = (float)(src->center[1] - sc.a_cen[1]), c2 = (float)(src->center[2] - sc.a_cen[2]);
    const float p00 = (float)src->rot_pos[0], p01 = (float)src->rot_pos[1], p10 = (float)src->rot_pos[3], p11 = (float)src->rot_pos[4],
                p20 = (float)src->rot_pos[6], p21 = (float)src->rot_pos[7];
    const float r00 = (float)src->rot_dir[0], r01 = (float)src->rot_dir[1], r02 = (float)src->rot_dir[2], r10 = (float)src->rot_dir[3],
                r11 = (float)src->rot_dir[4], r12 = (float)src->rot_dir[5], r20 = (float)src->rot_dir[6], r21 = (float)src->rot_dir[7],
                r22 = (float)src->rot_dir[8];
    const float t_adv = (float)F.t_adv;
    unsigned qh = 0, qt = 0;            // the queue holds entries qh .. qt - 1 (mod SFQ_CAP); the same in every lane
    // phase 2 on up to 64 entries of the queue: what k_s_fresh does for a listed ray
    auto phase2 = [&](const StreamParams &S, unsigned take) {
        const bool active = lane < take;
        uint32_t ri = 0, cell = 0;
        if (active) { ri = q_ray[(qh + lane) & (SFQ_CAP - 1)]; cell = q_cell[(qh + lane) & (SFQ_CAP - 1)]; }
        listed_ray_search<KIND, FLAT, LDS>(S, l_bf, recs, obb, l_coff, clist, cs, ch, active, ri, cell);
        qh += take;
    };
    // DERIVE: the instance finds a listed ray's mask cell itself, from the float32 start point of phase 1 (the cell k_s_cull packs:
    // the same functions on the same bits), and takes the list of k_s_ucull, which carries no cells.  The instances with the quadric
    // code in and their tables in global memory came out with 7 to 9 more vector registers that way: they are handed the cell.
    constexpr bool DERIVE = SF2_DERIVES_CELL(FLAT, LDS);
    uint32_t ri_n = SQ_INVALID, cell_n = 0;
    {
        const long long i0 = (long long)blockIdx.x * THREADS + threadIdx.x;
        if (i0 < count) { ri_n = W.fq_ray[i0]; if constexpr (!DERIVE) cell_n = W.fq_cell[i0]; }
    }
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < padded; i += (long long)gridDim.x * THREADS) {
        // the arguments of this turn: none of them lives across the loop in a scalar register
        const StreamParams *again = &S0;
        if constexpr (LDS) again = kernel_args_again<StreamParams>();
        const StreamParams &S = *again;
        const FastParams &P = S.P;
        const StreamWs &W = S.W;
        const trc_fp_params &F = S.fp.P;
        const uint32_t ri = ri_n;
        uint32_t cell = cell_n;
        {
            const long long i1 = i + (long long)gridDim.x * THREADS;
            ri_n = SQ_INVALID; cell_n = 0;
            if (i1 < count) { ri_n = W.fq_ray[i1]; if constexpr (!DERIVE) cell_n = W.fq_cell[i1]; }
        }
        const bool active = ri != SQ_INVALID;
        if (!__ballot(active)) continue;
        // phase 1: the ray in float32
        bool pass = false;
        {
            const unsigned long long rid = P.ray_offset + (unsigned long long)(S.base + ri);
            uint32_t o[4];
            trc_philox4x32_10((uint32_t)rid, (uint32_t)(rid >> 32), 0u, 0u, (uint32_t)P.seed, (uint32_t)(P.seed >> 32), o);
            float lx, ly;
            trc_fp_position32_t<KIND>(F, o, &lx, &ly);
            if constexpr (DERIVE) {
                int32_t ix, iy;
                trc_fp_cell(F, lx, ly, &ix, &iy);
                cell = ((uint32_t)iy << 16) | (uint32_t)ix;
            }
            const double u2 = ((double)o[2] + 0.5) * (1.0 / 4294967296.0);
            const float th = (float)trc_buie_theta_fast(l_bf, u2);
            float sxi, cxi;
            trc_fp_sincos_rev32(((float)o[3] + 0.5f) * (1.0f / 4294967296.0f), &sxi, &cxi);
            const float th2 = th * th;
            const float st = th * (1.0f - th2 * (1.0f / 6.0f)), ct = 1.0f - th2 * (0.5f - th2 * (1.0f / 24.0f));
            const float ax = cxi * st, ay = sxi * st, az = ct;
            const float ex = r00 * ax + r01 * ay + r02 * az, ey = r10 * ax + r11 * ay + r12 * az, ez = r20 * ax + r21 * ay + r22 * az;
            const float ox = c0 + p00 * lx + p01 * ly + t_adv * ex, oy = c1 + p10 * lx + p11 * ly + t_adv * ey, oz = c2 + p20 * lx + p21 * ly + t_adv * ez;
            uint32_t k0 = 0, k1 = 0;
            if (active) {
                const uint32_t c = ((cell >> 16) >> TRC_FP_SHIFT) * (uint32_t)F.Mc + ((cell & 0xFFFFu) >> TRC_FP_SHIFT);
                if (LDS) { k0 = l_coff[c]; k1 = l_coff[c + 1]; }
                else { k0 = S.fp.coff[c]; k1 = S.fp.coff[c + 1]; }
            }
            for (uint32_t k = k0; k < k1 && !pass; ++k)
                pass = trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * clist[k], ox, oy, oz, ex, ey, ez);
            pass = pass && active;
        }
        {
            const unsigned long long m = __ballot(pass);
            if (pass) {
                const unsigned at = (qt + (unsigned)__popcll(m & ((1ull << lane) - 1ull))) & (SFQ_CAP - 1);
                q_ray[at] = ri; q_cell[at] = cell;
            }
            qt += (unsigned)__popcll(m);
        }
        WAVE_SYNC();
        if (qt - qh >= 64u) { phase2(S, 64u); WAVE_SYNC(); }
    }
    const StreamParams *last = &S0;
    if constexpr (LDS) last = kernel_args_again<StreamParams>();
    while (qt != qh) { const unsigned take = qt - qh < 64u ? qt - qh : 64u; phase2(*last, take); }
    chunk_close(ch, last->W.hit_slot, SQ_ROOM(last->W));
}

// ---------------------------------------------------------------------------------------------------------------
// walk + balanced box tests, single precision only
// (SW_THREADS, SW_LEAFCAP, SW_LIST_T, SW_WAVE_BYTES: trc_forms.h)
#ifndef SW_ITEMS
#define SW_ITEMS 4
#endif

struct WalkLds {
    uint32_t *stack;   // [depth][64]
    SW_LIST_T *lst;    // [SW_LEAFCAP][64]
    uint32_t *pre;     // [64]
};

// list entries are Kd leaf nodes (goff == nullptr) or grid cells (offsets in goff)
__device__ __forceinline__ void sw_drain(const trc_accel_view &A, const float *obb, const uint16_t *goff, const WalkLds &L, const StreamWs &W, WaveChunk &c3,
                                         unsigned cnt, const trc_ray32 &mine, uint32_t my_slot, unsigned lane) {
    unsigned incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    const unsigned total = __shfl(incl, 63, 64);
    if (total == 0) return;
#ifdef SW_STATS
    if (lane == 0) { atomicAdd(&W.cnt[CN(CW_STATS + 5)], 1ull); atomicAdd(&W.cnt[CN(CW_STATS + 6)], (unsigned long long)((total + 63) / 64)); }
#endif
    L.pre[lane] = incl;
    WAVE_SYNC();
    for (unsigned base = 0; base < total; base += 64) {
        const unsigned e = base + lane;
        const bool valid = e < total;
        unsigned lc = 0, off = 0, owner = 0;
        if (valid) {
            unsigned lo = 0, hi = 63;
            while (lo < hi) {
                unsigned mid = (lo + hi) >> 1;
                if (L.pre[mid] > e) hi = mid; else lo = mid + 1;
            }
            owner = lo;
            unsigned j = e - (owner ? L.pre[owner - 1] : 0u);
            unsigned node = L.lst[j * 64 + owner];
            if (goff) { off = goff[node]; lc = (unsigned)goff[node + 1] - off; }
            else { off = A.nodes[2 * node]; lc = A.nodes[2 * node + 1] >> 2; }
        }
        trc_ray32 r;
        r.ox = __shfl(mine.ox, (int)owner, 64); r.oy = __shfl(mine.oy, (int)owner, 64); r.oz = __shfl(mine.oz, (int)owner, 64);
        r.ix = __shfl(mine.ix, (int)owner, 64); r.iy = __shfl(mine.iy, (int)owner, 64); r.iz = __shfl(mine.iz, (int)owner, 64);
        r.dx = __builtin_amdgcn_rcpf(r.ix); r.dy = __builtin_amdgcn_rcpf(r.iy); r.dz = __builtin_amdgcn_rcpf(r.iz);   // 1 / (1 / d): 2 ulp, 0 stays 0
        const uint32_t oslot = (uint32_t)__shfl((int)my_slot, (int)owner, 64);
        for (unsigned kb = 0; __ballot(kb < lc); kb += 32) {
            unsigned hits = 0;
            for (unsigned k0 = kb; k0 < kb + 32 && __ballot(k0 < lc); k0 += 4) {
                unsigned sid[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sid[q] = (k0 + q < lc) ? (unsigned)A.leaf_surfs[off + k0 + q] : 0u;
                bool h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h[q] = trc_box_hit32(A.sbox + 6 * (size_t)sid[q], r);
#pragma unroll
                for (int q = 0; q < 4; ++q) if (h[q] && k0 + q < lc) hits |= 1u << (k0 + q - kb);
            }
            while (__ballot(hits != 0)) {
                bool want = hits != 0;
                unsigned k = want ? kb + (unsigned)__ffs((int)hits) - 1u : 0u;
                unsigned sidx = want ? (unsigned)A.leaf_surfs[off + k] : 0u;
                // the surface's own (oriented) box: for a plate the plate itself +- delta -- three of four rays that cross the
                // axis-aligned box of a tilted mirror miss the mirror
                if (want) want = trc_obb_hit32(obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
                unsigned long long q3 = chunk_append(&W.cnt[CN(CW_Q3)], c3, want, W.q3_slot, W.q3_cap);
                if (want) {
                    if ((long long)q3 < W.q3_cap) { W.q3_slot[q3] = oslot; W.q3_surf[q3] = sidx; }
                    else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_RETRY;
                }
                hits &= hits - 1u;
            }
        }
    }
    WAVE_SYNC();
}

// GRID: the uniform-grid instance carries no tree code -- the Kd step picks ray components by axis number, which the
// compiler serves from a copy of the ray in scratch memory (36 bytes per lane written at every wave iteration: 1.2 GB per
// 1e8 rays when the two shared a kernel)
template <int THREADS, bool GRID>
__global__ __launch_bounds__(THREADS) void k_s_walk(StreamParams S) {
    extern __shared__ double lds[];
    const DScene &sc = S.P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    const int tid = threadIdx.x;
    const unsigned lane = lane_id();
    const int mode = GRID ? 2 : S.search;
    const bool kd32 = mode == 1;
    trc_accel_view A = stream_accel_global(sc, mode);
    WalkLds L;
    trc_grid_view G;
    const uint16_t *goff = nullptr;
    {
        float *l_sbox = (float *)lds;
        for (int i = tid; i < 6 * Sn; i += THREADS) l_sbox[i] = sc.a_sbox[i];
        char *cur = (char *)(l_sbox + 6 * Sn);
        uint32_t *l_nodes = (uint32_t *)cur;
        uint16_t *l_leaf;
        if (mode == 2) {
            uint16_t *l_goff = (uint16_t *)cur;
            for (int i = tid; i < sc.a_g_ncell + 1; i += THREADS) l_goff[i] = sc.a_goff[i];
            l_leaf = l_goff + ((sc.a_g_ncell + 2) & ~1);
            for (int i = tid; i < sc.a_g_nlist; i += THREADS) l_leaf[i] = sc.a_glist[i];
            cur = (char *)(l_leaf + sc.a_g_nlist);
            goff = l_goff;
            G.off = l_goff; G.list = l_leaf;
            G.nx = sc.a_gdim[0]; G.ny = sc.a_gdim[1]; G.nz = sc.a_gdim[2];
            G.lox = sc.a_glo[0]; G.loy = sc.a_glo[1]; G.loz = sc.a_glo[2];
            G.csx = sc.a_gcs[0]; G.csy = sc.a_gcs[1]; G.csz = sc.a_gcs[2];
            G.ivx = sc.a_ginv[0]; G.ivy = sc.a_ginv[1]; G.ivz = sc.a_ginv[2];
        } else {
            const int nn = kd32 ? sc.kd_nodes : 1;
            for (int i = tid; i < 2 * nn; i += THREADS) l_nodes[i] = kd32 ? sc.a_nodes[i] : sc.a_bnodes[i];
            l_leaf = (uint16_t *)(l_nodes + 2 * nn);
            const int nl = kd32 ? sc.kd_nleaf : sc.a_n_bleaf;
            for (int i = tid; i < nl; i += THREADS) l_leaf[i] = kd32 ? sc.a_leaf[i] : sc.a_bleaf[i];
            cur = (char *)(l_leaf + nl);
        }
        size_t off = (size_t)(cur - (char *)lds);
        off = (off + 15) & ~(size_t)15;
        const int depth = kd32 ? (sc.a_kd_depth > 0 ? sc.a_kd_depth : 1) : 1;
        char *wb = (char *)lds + off + (size_t)(tid >> 6) * SW_WAVE_BYTES(depth);
        L.stack = (uint32_t *)wb; wb += (size_t)depth * 64 * 4;
        L.pre = (uint32_t *)wb; wb += 64 * 4;
        L.lst = (SW_LIST_T *)wb;
        A.sbox = l_sbox; A.nodes = l_nodes; A.leaf_surfs = l_leaf;
    }
    __syncthreads();
    if (W.cnt[CN(CW_OVERFLOW)] == CW_OVF_FAIL) return;       // a list overflowed upstream: the host gives the call up, nothing below may run on its leftovers
    long long nq = (long long)W.cnt[CN(CW_Q1)];
    if (nq > SQ_ROOM(W)) nq = SQ_ROOM(W);   // never read beyond the allocation, whatever the counter says
    const long long n_waves = (long long)gridDim.x * (THREADS >> 6);
    const long long wave = (long long)blockIdx.x * (THREADS >> 6) + (tid >> 6);
    WaveChunk c3 = S.static_general ? chunk_init_static(S.chunk_q3, (unsigned long long)wave) : chunk_init(S.chunk_q3);
    for (long long wbase = wave * 64; wbase < nq; wbase += n_waves * 64) {
        const long long i = wbase + lane;
        const bool valid = i < nq;
        trc_ray32 r;
        r.ox = r.oy = r.oz = r.ix = r.iy = r.iz = r.dx = r.dy = r.dz = 0.0f;
        float tmin = 1.0f, tmax = 0.0f;
        uint32_t slot = 0;
        if (valid) {
            slot = W.q1_slot[i];
            if (slot != SQ_INVALID) {
                float4 a = W.q1_a[i], b = W.q1_b[i];
                r.ox = a.x; r.oy = a.y; r.oz = a.z; r.ix = a.w; r.iy = b.x; r.iz = b.y; tmin = b.z; tmax = b.w;
            }
        }
        bool walk = valid && slot != SQ_INVALID && (tmax >= tmin);
        uint32_t node = 0;
        int sp = 0;
        unsigned cnt = 0;
#ifdef SW_STATS
        if (walk) atomicAdd(&W.cnt[CN(CW_STATS)], 1ull);
#endif
        if (GRID) {
            // uniform grid: list the non-empty cells of the DDA between tmin and tmax
            trc_dda dd;
            dd.cx = dd.cy = dd.cz = 0; dd.tnx = dd.tny = dd.tnz = 0.0f;
            if (walk) trc_dda_start(G, r, tmin, &dd);
            while (__ballot(walk)) {
#pragma unroll 1
                for (int rep = 0; rep < 4 && walk && cnt < SW_LEAFCAP; ++rep) {
                    const int cell = trc_dda_cell(G, dd);
#ifdef SW_STATS
                    atomicAdd(&W.cnt[CN(CW_STATS + 2)], 1ull);
                    if (goff[cell + 1] != goff[cell]) { atomicAdd(&W.cnt[CN(CW_STATS + 3)], 1ull); atomicAdd(&W.cnt[CN(CW_STATS + 4)], (unsigned long long)(goff[cell + 1] - goff[cell])); }
#endif
                    if (goff[cell + 1] != goff[cell]) { L.lst[cnt * 64 + lane] = (SW_LIST_T)cell; ++cnt; }
                    walk = trc_dda_next(G, r, tmax, &dd);
                }
                if (__ballot(cnt >= SW_LEAFCAP)) {
                    sw_drain(A, sc.a_obb, goff, L, W, c3, cnt, r, slot, lane);
                    cnt = 0;
                }
            }
        }
        while (!GRID && __ballot(walk)) {
#ifdef SW_STATS
            if (lane == 0) atomicAdd(&W.cnt[CN(CW_STATS + 1)], 1ull);
#endif
#pragma unroll 1
            for (int rep = 0; rep < 4 && walk && cnt < SW_LEAFCAP; ++rep) {
                uint32_t w0 = A.nodes[2 * node], w1 = A.nodes[2 * node + 1];
#ifdef SW_STATS
                atomicAdd(&W.cnt[CN(CW_STATS + 2)], 1ull);
                if ((w1 & 3u) == 3u && (w1 >> 2) != 0u) { atomicAdd(&W.cnt[CN(CW_STATS + 3)], 1ull); atomicAdd(&W.cnt[CN(CW_STATS + 4)], (unsigned long long)(w1 >> 2)); }
#endif
                if ((w1 & 3u) != 3u) {
                    bool push;
                    uint32_t na;
                    float pt;
                    node = trc_kd32_step(w0, w1, r, A.delta, tmin, &tmax, &push, &na, &pt);
                    if (push) {
                        uint32_t bts = __float_as_uint(pt);
                        uint32_t hb = (bts >> 16) + ((bts & 0xFFFFu) ? 1u : 0u);   // interval end rounded up: conservative
                        L.stack[sp * 64 + lane] = (na << 16) | (hb & 0xFFFFu);
                        ++sp;
                    }
                } else {
                    if ((w1 >> 2) != 0u) { L.lst[cnt * 64 + lane] = (SW_LIST_T)node; ++cnt; }
                    if (sp == 0) walk = false;
                    else {
                        --sp;
                        uint32_t en = L.stack[sp * 64 + lane];
                        uint32_t na = en >> 16;
                        node = na >> 2;
                        tmin = trc_kd32_pop_tmin(na & 3u, r, A.delta, tmax);
                        tmax = __uint_as_float(en << 16);
                    }
                }
            }
            if (__ballot(cnt >= SW_LEAFCAP)) {
                sw_drain(A, sc.a_obb, goff, L, W, c3, cnt, r, slot, lane);
                cnt = 0;
            }
        }
        sw_drain(A, sc.a_obb, goff, L, W, c3, cnt, r, slot, lane);
    }
    chunk_close(c3, W.q3_slot, W.q3_cap);
}

// ---------------------------------------------------------------------------------------------------------------
// A continued ray's whole search in one kernel, one lane per ray (bounces >= 1 on the grid or the all-boxes form): re-entry
// into the scene box, the surfaces set apart, the cells of the DDA with their surfaces -- axis-aligned box, oriented box,
// exact float64 test -- and the nearest hit with the reference's tie rule kept in registers; the ray is appended to the hit
// list with its surface and distance.  Rays of the later bounces were aimed (a heliostat field sends them to one receiver):
// they have one or two candidates and a few cells each, so the lanes of a wave run alike, and the walker / candidate queues,
// the linking of candidates per ray with atomics and three kernel boundaries per bounce cost more than they balance
// (k_s_gen<false> + k_s_walk + k_s_exact: 0.92 ms per 3.2e6 NSTTF rays; this kernel: see profiles/).  The walk ends at the
// first cell that starts behind the best hit: a surface is listed in every cell its box overlaps, the cell of a nearer hit
// has been visited.

// GRIDM: 0 every bounded surface (accel = False), 1 the grid that fits LDS, 2 the 32-bit grid of large scenes (global memory),
// 3 scenes of a few surfaces (a dish and its receiver, a cavity of seven walls), surface by surface: the wave goes through the
// surfaces together, every lane whose ray passes the surface's boxes runs the exact test of that ONE surface.  Its record is
// then the same for all lanes -- read through the scalar cache into scalar registers -- and its kind is decided by a scalar
// branch, where lanes that each test "their" next candidate run the code of every kind present one after the other (the
// seven-wall cavity: frustum, cylinder, cone and three discs in one wave).  No tables in LDS (LDS = false).
// LDS: all tables of the search staged in LDS, or none (see k_s_fresh).
// FRESH: the rays are generated here instead of read from the table -- k_s_gen + k_s_walk + k_s_exact in one kernel for the fresh rays
// that the footprint map does not cover (the Buie aureole, sources it does not apply to, given bundles) in scenes whose search
// structures do not fit the LDS of the walk kernel (meshes of 1e5 faces), or everywhere with TRC_STREAM_FIRST=1.  A ray that hits
// takes the next slot of the table.
// FLAT: every surface of the scene is of a flat kind: no quadric code in the exact test (as in k_s_fresh).
// (SB_THREADS, and the LDS image of k_s_bounce / k_s_bounce_coop, bounce_lds_parts: trc_forms.h)
#ifdef SB_STATS      /* diagnostic builds only: what the lanes of k_s_bounce spend their turns on (printed at the end of a call) */
__device__ unsigned long long g_sb_stats[32];        /* [0, 16): fresh rays, [16, 32): continued rays */
#define SB_COUNT(K, V) atomicAdd(&g_sb_stats[(FRESH ? 0 : 16) + (K)], (unsigned long long)(V))
#else
#define SB_COUNT(K, V) ((void)0)
#endif
// SUN: a FRESH instance for the tabulated sunshapes (trc_source_ray_t)
template <int GRIDM, bool LDS, bool FRESH, bool FLAT = false, bool SUN = false>
__global__ __launch_bounds__(SB_THREADS_OF(GRIDM)) void k_s_bounce(StreamParams S0) {
    constexpr int THREADS = SB_THREADS_OF(GRIDM);
    extern __shared__ double lds[];
    constexpr bool GRID = GRIDM == 1 || GRIDM == 2;
    typedef typename std::conditional<GRIDM == 2, trc_grid_view32, trc_grid_view>::type grid_t;
    // (one explicit argument: kernel_args_again.  AGAIN: the instance reads its arguments again in every turn of its loop and builds
    // its views of them there -- the continued rays on the LDS-sized grid and on all boxes.  The FRESH instances, the large grid, the
    // surface-by-surface form and the all-boxes instance with quadrics and its tables in global memory came out with more vector
    // registers or scratch that way: they keep the views made here from the by-value block, as before)
    constexpr bool AGAIN = !FRESH && (GRIDM == 1 || (GRIDM == 0 && (LDS || FLAT)));
    const StreamParams &S = S0;
    const FastParams &P = S.P;
    const DScene &sc = S.P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    const int tid = threadIdx.x;
    trc_accel_view A0 = stream_accel_global(sc, GRIDM == 1 ? 2 : 0);
    if (GRIDM == 2) {           // the large grid and the few surfaces set apart from it
#pragma unroll
        for (int i = 0; i < 6; ++i) A0.root[i] = sc.a_bg_root[i];
        A0.always = sc.a_bg_apart;
        A0.n_always = sc.a_bg_napart;
    }
    const double *recs0 = sc.recs;
    const float *obb0 = sc.a_obb;
    const int32_t *sflags = sc.sflags;
    grid_t G0;
    memset(&G0, 0, sizeof(G0));
    if (GRIDM == 1) {
        G0.off = (decltype(G0.off))sc.a_goff; G0.list = (decltype(G0.list))sc.a_glist;
        G0.nx = sc.a_gdim[0]; G0.ny = sc.a_gdim[1]; G0.nz = sc.a_gdim[2];
        G0.lox = sc.a_glo[0]; G0.loy = sc.a_glo[1]; G0.loz = sc.a_glo[2];
        G0.csx = sc.a_gcs[0]; G0.csy = sc.a_gcs[1]; G0.csz = sc.a_gcs[2];
        G0.ivx = sc.a_ginv[0]; G0.ivy = sc.a_ginv[1]; G0.ivz = sc.a_ginv[2];
    }
    if (GRIDM == 2) {
        G0.off = (decltype(G0.off))sc.a_bg_off; G0.list = nullptr;       // (the lists: sc.a_bg_ent)
        G0.nx = sc.a_bg_dim[0]; G0.ny = sc.a_bg_dim[1]; G0.nz = sc.a_bg_dim[2];
        G0.lox = sc.a_bg_lo[0]; G0.loy = sc.a_bg_lo[1]; G0.loz = sc.a_bg_lo[2];
        G0.csx = sc.a_bg_cs[0]; G0.csy = sc.a_bg_cs[1]; G0.csz = sc.a_bg_cs[2];
        G0.ivx = sc.a_bg_inv[0]; G0.ivy = sc.a_bg_inv[1]; G0.ivz = sc.a_bg_inv[2];
    }
    // dynamic LDS: [the Buie tables (FRESH)] [occupancy bits (large grid)] [records | oriented boxes | boxes | flags | grid (LDS)]
    char *cur = (char *)lds;
    trc_buie_fast *l_bf = nullptr;
    const uint32_t *occ = sc.a_bg_occ;
    if constexpr (GRIDM == 2) {
        // (the large grid has no tables in LDS: its two parts are carved here, in the layout's order -- through the layout the
        // instances of this form changed their scratch)
        if (FRESH) { l_bf = (trc_buie_fast *)cur; cur += (sizeof(trc_buie_fast) + 15) & ~(size_t)15; }
        // one bit per cell that lists anything, in LDS when the host found room for it -- most cells of a ray's way are empty, and
        // a step through one then reads nothing from memory
        if (S.bg_occ_words > 0) {
            uint32_t *l_occ = (uint32_t *)cur; cur += (((size_t)S.bg_occ_words * 4) + 15) & ~(size_t)15;
            for (int i = tid; i < S.bg_occ_words; i += THREADS) l_occ[i] = sc.a_bg_occ[i];
            occ = l_occ;
        }
    } else {
        const trc_lds_parts parts = bounce_lds_parts(Sn, sc.stride, FRESH, LDS, LDS && !FRESH, (LDS && GRIDM == 1) ? sc.a_g_ncell : 0, sc.a_g_nlist, 0, 0);
        const trc_lds_layout L = trc_search_lds_layout(parts);
        if (FRESH) l_bf = (trc_buie_fast *)(cur + L.buie);
        stage_search_tables<THREADS>(cur, L, parts, sc, S.fp, tid);
        if (LDS) {
            recs0 = (const double *)(cur + L.recs); obb0 = (const float *)(cur + L.obb);
            A0.sbox = (const float *)(cur + L.sbox);
            if (!FRESH) sflags = (const int32_t *)(cur + L.flags);
            if (GRIDM == 1) { G0.off = (decltype(G0.off))(cur + L.grid_off); G0.list = (decltype(G0.list))(cur + L.grid_list); }
        }
        cur += L.end;
    }
    // split_terminal == 2: the hits on surfaces that end every ray are finished HERE (what k_s_absorb does behind a list: hit point,
    // tallies, flux-map bin, hit capture) -- the list entry, its re-read, the second read of the ray record and a launch less per
    // bounce.  Tallies, flux-map tables and bins of the workgroup in LDS behind the tables of the search.
    const bool absorb_here = !FRESH && S.split_terminal == 2;
    DScene La0 = sc;      // (the workgroup's view for the hits it finishes: its copy of the tally buffer, the tables in LDS)
    double *a_tally = nullptr, *a_fm = nullptr;
    if (absorb_here) {
        // (the image of TRC_IMG_INLINE, trc_shade_lds_layout in trc_bounds.h, by which the host sizes it: carved here in its order, on the
        // next 16 bytes behind the search image -- through a shared staging routine two instances spilled more scalar registers)
        cur = (char *)(((uintptr_t)cur + 15) & ~(uintptr_t)15);
        La0.tally = W.tally_part + (size_t)(blockIdx.x % TALLY_PARTS) * (size_t)W.tally_n;
        a_tally = (double *)cur; cur += (size_t)(3 * Sn + 2) * 8;
        for (int i = tid; i < 3 * Sn + 2; i += THREADS) a_tally[i] = 0.0;
        double *l_edges = (double *)cur; cur += (size_t)sc.n_fm_edges * 8;
        for (int i = tid; i < sc.n_fm_edges; i += THREADS) l_edges[i] = sc.fm_edges[i];
        FluxMapDev *l_fms = (FluxMapDev *)cur; cur += ((sc.n_fm * sizeof(FluxMapDev) + 7) / 8) * 8;
        for (int i = tid; i < sc.n_fm; i += THREADS) l_fms[i] = sc.fms[i];
        int32_t *l_fm_of = (int32_t *)cur; cur += (((size_t)Sn * 4) + 7) & ~(size_t)7;
        for (int i = tid; i < Sn; i += THREADS) l_fm_of[i] = sc.fm_of_surf ? sc.fm_of_surf[i] : -1;
        La0.fm_edges = l_edges; La0.fms = l_fms; La0.fm_of_surf = l_fm_of; La0.sflags = sflags;
        if (S.lds_fm_bins > 0) {
            a_fm = (double *)cur; cur += (size_t)S.lds_fm_bins * 8;
            for (int i = tid; i < S.lds_fm_bins; i += THREADS) a_fm[i] = 0.0;
        }
    }
    const unsigned wave_a = (unsigned)(((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    WaveChunk hc = chunk_init(S.chunk_hitbuf);          // this wave's open chunk of the scene's hit buffer (see k_s_shade)
    if (absorb_here && P.capture && wave_a < SHADE_MAX_WAVES) hit_chunk_resume(hc, W.hit_state + 2 * wave_a, S.hit_epoch);
    unsigned n_term = 0;
    const bool buie_src = FRESH && P.src && (P.src->kind == TRC_SRC_BUIE_DISK || P.src->kind == TRC_SRC_BUIE_RECT);
    if (FRESH) buie_tables_fill(P.src, l_bf, tid, THREADS, buie_src);
    else __syncthreads();
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    // the rays: the active list (slots), or fresh rays by number -- all of the batch or those k_s_cull left to this path
    const uint32_t *list = FRESH ? S.gen_list : S.act_in;
    long long count = FRESH ? (list ? (long long)W.cnt[CN(CW_GEN_LIST)] : S.nb) : (long long)W.cnt[CN(CW_ACT_IN)];
    if (list && count > (FRESH ? SQ_ROOM(W) : W.act_room)) count = FRESH ? SQ_ROOM(W) : W.act_room;
    const long long padded = (count + 63) & ~63ll;
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    // fresh rays: pre-assigned chunks behind those of k_s_fresh (hit_base0 / slot_base0), SQ_CHUNK each
    WaveChunk ch = S.static_first ? (FRESH ? chunk_init_static_at(S.chunk_first, (unsigned long long)S.hit_base0 + wave_g * S.chunk_first) : chunk_init_static(S.chunk_hit, wave_g))
                                  : chunk_init(FRESH ? S.chunk_first : S.chunk_hit);
    WaveChunk cs = (FRESH && S.static_first) ? chunk_init_static_at(S.chunk_first, (unsigned long long)S.slot_base0 + wave_g * S.chunk_first) : chunk_init(S.chunk_first);
    // hits on surfaces that end every ray go to a list of their own (k_s_absorb: no optics to sample, a quarter of the registers)
    const bool split = !FRESH && S.split_terminal;
    WaveChunk ct = (split && S.static_first) ? chunk_init_static(S.chunk_thit, wave_g) : chunk_init(S.chunk_thit);
    // the entry of the active list for the next iteration is fetched while this one is worked on: the list entry and the ray record
    // behind it are two round trips in a row otherwise
    const long long bstride = (long long)gridDim.x * blockDim.x;
    uint32_t slot_next = SQ_INVALID;
    if (!FRESH) { const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; if (i0 < count) slot_next = S.act_in[i0]; }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += bstride) {
        // the arguments of this turn and the views made of them (AGAIN: read again, none of them lives across the loop)
        const StreamParams *again = &S0;
        if constexpr (AGAIN) again = kernel_args_again<StreamParams>();
        const StreamParams &S = *again;
        const FastParams &P = S.P;
        const DScene &sc = S.P.sc;
        const StreamWs &W = S.W;
        const uint32_t *list = FRESH ? S.gen_list : S.act_in;
        // (AGAIN: what does not come from the workgroup's LDS is taken from the arguments of this turn; else the views made above)
        trc_accel_view A_t;
        grid_t G_t;
        DScene La_t;
        if constexpr (AGAIN) {
            A_t = stream_accel_global(sc, GRIDM == 1 ? 2 : 0);
            if (LDS) A_t.sbox = A0.sbox;
            memset(&G_t, 0, sizeof(G_t));
            if (GRIDM == 1) {
                G_t.off = LDS ? G0.off : (decltype(G_t.off))sc.a_goff; G_t.list = LDS ? G0.list : (decltype(G_t.list))sc.a_glist;
                G_t.nx = sc.a_gdim[0]; G_t.ny = sc.a_gdim[1]; G_t.nz = sc.a_gdim[2];
                G_t.lox = sc.a_glo[0]; G_t.loy = sc.a_glo[1]; G_t.loz = sc.a_glo[2];
                G_t.csx = sc.a_gcs[0]; G_t.csy = sc.a_gcs[1]; G_t.csz = sc.a_gcs[2];
                G_t.ivx = sc.a_ginv[0]; G_t.ivy = sc.a_ginv[1]; G_t.ivz = sc.a_ginv[2];
            }
            La_t = sc;
            La_t.tally = La0.tally; La_t.fm_edges = La0.fm_edges; La_t.fms = La0.fms; La_t.fm_of_surf = La0.fm_of_surf; La_t.sflags = La0.sflags;
        }
        const trc_accel_view &A = AGAIN ? A_t : A0;
        const grid_t &G = AGAIN ? G_t : G0;
        const DScene &La = AGAIN ? La_t : La0;
        const double *recs = (AGAIN && !LDS) ? sc.recs : recs0;
        const float *obb = (AGAIN && !LDS) ? sc.a_obb : obb0;
        uint32_t *const t_slot = W.q1_slot;
        uint32_t *const t_surf = (uint32_t *)W.q1_a;
        double *const t_t = (double *)W.q1_b;
        uint32_t slot = SQ_INVALID, ri = SQ_INVALID;
        if (FRESH) { if (i < count) ri = list ? list[i] : (uint32_t)i; }
        else {
            slot = slot_next;
            asm volatile("" : "+v"(slot));          // (arrives here, before the next one is asked for: see k_s_shade)
            slot_next = SQ_INVALID;
            if (i + bstride < count) slot_next = S.act_in[i + bstride];
        }
        const bool valid = FRESH ? ri != SQ_INVALID : slot != SQ_INVALID;
        if (!__ballot(valid)) continue;
        if (valid) SB_COUNT(7, 1);
        if (lane_id() == 0) SB_COUNT(9, 1);
        double tb = TRC_INF;
        int sb = 0x7FFFFFFF;
        double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 1, e0 = 0, ref0 = 1.0, wl0 = 0.0;
        int skip = -1;                // the surface the ray left, when it cannot meet it again
        int left = Sn;                // the surface the ray left (Sn: the source)
        if (valid) {
            if (FRESH) {
                unsigned long long rid;
                fast_new_ray<-1, false, SUN>(P, nullptr, S.base + ri, px, py, pz, dx, dy, dz, e0, ref0, wl0, rid, buie_src ? l_bf : nullptr);
            } else {
                const SRayGeo g = W.geo[slot];
                px = g.px; py = g.py; pz = g.pz; dx = g.dx; dy = g.dy; dz = g.dz;
                const uint32_t pw = (uint32_t)(g.tail >> 32);
                if (pw & SQ_SKIP_SELF) skip = (int)(pw & ~SQ_SKIP_SELF);
                if ((uint32_t)g.tail != 0u) left = (int)(pw & ~SQ_SKIP_SELF);
            }
        }
        // Candidates that pass their boxes wait in a small list of the lane (4 x 16 bits) and are tested exactly by all lanes
        // together (sb_flush): an exact float64 test run by the few lanes that happen to need one at the same point of the walk
        // stalls the other lanes for its whole length.  A fifth candidate is tested on the spot.
        // (the large grid serves scenes of up to 2^21 surfaces: 3 x 21 bits there)
        constexpr int CL_BITS = GRIDM == 2 ? 21 : 16, CL_CAP = GRIDM == 2 ? 3 : 4;
        const bool SB_WIDE_TRI = GRIDM == 2 && sc.stride >= 20;      // (the large grid: meshes)
        unsigned long long cl = 0ull;
        int nc = 0;
#define SB_TEST(SIDX)                                                                                                   \
        do {                                                                                                            \
            const int _s = (int)(SIDX);                                                                                 \
            SB_COUNT(3, 1);                                                                                             \
            const double *_rec = recs + (size_t)_s * sc.stride;                                                         \
            double _t;                                                                                                  \
            if (SB_WIDE_TRI) {      /* the whole record of a triangular face (20 doubles) in ten 16-byte loads: a   */ \
                                    /* record starts on 8 bytes (odd stride), which global loads of 16 bytes accept */ \
                double _l[20];                                                                                          \
                const double2 *_q = (const double2 *)_rec;                                                              \
                _Pragma("unroll") for (int _k = 0; _k < 10; ++_k) { const double2 _v = _q[_k]; _l[2 * _k] = _v.x; _l[2 * _k + 1] = _v.y; } \
                const int _kind = trc_rec_gm_kind(_l);                                                                  \
                _t = _kind == TRC_GM_TRIANGLE ? trc_intersect_flat(TRC_GM_TRIANGLE, _l, sc.extra, px, py, pz, dx, dy, dz) \
                   : (FLAT ? trc_intersect_flat(_kind, _rec, sc.extra, px, py, pz, dx, dy, dz)                          \
                           : trc_intersect(_rec, sc.extra, px, py, pz, dx, dy, dz));                                    \
            } else                                                                                                      \
            _t = FLAT ? trc_intersect_flat(trc_rec_gm_kind(_rec), _rec, sc.extra, px, py, pz, dx, dy, dz)               \
                      : trc_intersect(_rec, sc.extra, px, py, pz, dx, dy, dz);                                          \
            if (_t > 0.0 && _t < TRC_INF && (_t < tb || (_t == tb && _s < sb))) { tb = _t; sb = _s; }                   \
        } while (0)
#define SB_PUSH(SIDX)                                                                                                   \
        do {                                                                                                            \
            const int _p = (int)(SIDX);                                                                                 \
            if (_p != skip) {                                                                                           \
                if (Sn <= (1 << CL_BITS) && nc < CL_CAP) { cl |= (unsigned long long)(unsigned)_p << (CL_BITS * nc); ++nc; } \
                else SB_TEST(_p);                                                                                       \
            }                                                                                                           \
        } while (0)
#define SB_FLUSH_ROUND()                                                                                                \
        do {                                                                                                            \
            if (lane_id() == 0) SB_COUNT(6, 1);                                                                         \
            if (nc > 0) { const int _f = (int)(cl & ((1ull << CL_BITS) - 1)); cl >>= CL_BITS; --nc; SB_TEST(_f); }      \
        } while (0)
#define SB_FLUSH()                                                                                                      \
        while (__ballot(nc > 0)) SB_FLUSH_ROUND();
        trc_ray32 r;
        double t0 = 0.0;
        bool in = false, walk = false;
        float tmin = 1.0f, tmax = 0.0f;
        if (GRIDM == 3) {
            if (valid) in = trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0);
            for (int s = 0; s < Sn; ++s) {             // ascending: on equal t the lowest index stays (tracer_engine.py:58-63)
                const float *b = sc.a_sbox + 6 * (size_t)s;
                const bool unbounded = b[3] == TRC_INF && b[0] == -TRC_INF;
                bool cand = valid && s != skip;
                if (cand && !unbounded)
                    cand = in && trc_box_hit32(b, r) && trc_obb_hit32(sc.a_obb + (size_t)TRC_OBB_STRIDE * s, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
                if (__ballot(cand)) {
                    if (cand) SB_TEST(s);
                }
            }
        } else
        if (valid) {
            for (int k = 0; k < A.n_unbounded; ++k) SB_PUSH(A.unbounded[k]);
            in = trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0);
            if (in) {
                for (int k = 0; k < A.n_always; ++k) {        // surfaces set apart from the grid
                    const int sidx = A.always[k];
                    const float *b = A.sbox + 6 * (size_t)sidx;
                    if (b[3] == TRC_INF && b[0] == -TRC_INF) continue;
                    if (trc_box_hit32(b, r) && trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) SB_PUSH(sidx);
                }
                walk = trc_kd32_root(A.root, r, &tmin, &tmax);
                // A continued ray inside the clear cone of the tile it left (trc_clear_build) can meet the box of no surface the grid
                // lists: it does not walk.  The heliostats' rays to the receiver: all but one in 180 on NSTTF.
                // (k_s_shade_c's AHEAD, trc_shade.hip, restates this test, the tests of the surfaces set apart above and the terminal
                // hits finished below for the rays it finishes itself: whoever changes one of the two changes the other)
                if constexpr (GRIDM == 1 && !FRESH) {
                    if (walk && skip >= 0 && S.clear_tab && t0 == 0.0) {
                        const int tile = trc_clear_tile(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * skip, TRC_CLEAR_T, r.ox, r.oy, r.oz);
                        const float4 cone = ((const float4 *)S.clear_tab)[(size_t)skip * (TRC_CLEAR_T * TRC_CLEAR_T) + tile];
                        if (trc_clear_inside(cone.x, cone.y, cone.z, cone.w, r.dx, r.dy, r.dz)) { walk = false; SB_COUNT(10, 1); }
                    }
                }
            }
        }
        SB_FLUSH();         // the hit on a surface set apart (the receiver of a field) bounds the walk below
        if (GRID) {
            trc_dda dd;
            dd.cx = dd.cy = dd.cz = 0; dd.tnx = dd.tny = dd.tnz = 0.0f;
            if (walk) trc_dda_start(G, r, tmin, &dd);
            float t_enter = tmin;
            if (GRIDM == 2) {
                // The large grid (a mesh): cells hold half a dozen faces and a ray steps through a dozen cells, most of them empty.  A
                // lane either tests ONE listed surface of its cell or steps to its next cell that lists anything (four cells at most)
                // per turn of the loop, so that a wave takes as many turns as its busiest lane has occupied cells plus candidates --
                // with the list of a cell walked inside the step, it took the longest list of the wave at every step (12 to 14
                // thousand vector instructions per 64 rays on the relief of 1e5 faces).  What a candidate is tested with comes with
                // its list entry (48 bytes: a triangle's corner and edges, another kind's box), and the entry behind it is on its
                // way while this one is tested: entry -> box -> oriented box were three round trips one behind the other.
                const float4 *ent = (const float4 *)sc.a_bg_ent;
                unsigned kc = 0, kc1 = 0;
                float4 n0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n1 = n0, n2 = n0;
                while (__ballot(walk || kc < kc1)) {
                    if (lane_id() == 0) SB_COUNT(5, 1);
                    if (kc < kc1) {
                        SB_COUNT(1, 1);
                        const float4 c0 = n0, c1 = n1, c2 = n2;
                        ++kc;
                        if (kc < kc1) { n0 = ent[3 * (size_t)kc]; n1 = ent[3 * (size_t)kc + 1]; n2 = ent[3 * (size_t)kc + 2]; }
                        const uint32_t w = __float_as_uint(c0.x);
                        const int sidx = (int)(w & 0x7FFFFFFFu);
                        if (sidx != skip) {
                            bool pass;
                            if (!(w & 0x80000000u)) pass = trc_tri_hit32(c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, A.delta, r);
                            else {
                                const float b[6] = {c0.y, c0.z, c0.w, c1.x, c1.y, c1.z};
                                pass = trc_box_hit32(b, r) && trc_obb_hit32(obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
                            }
                            if (pass) { SB_COUNT(2, 1); SB_PUSH(sidx); }
                        }
                    } else if (walk) {
                        if (sb != 0x7FFFFFFF) {
                            const float tbr = (float)(tb - t0);
                            if (tbr < t_enter - (1e-3f + 1e-4f * fabsf(tbr))) walk = false;    // every cell from here on starts behind the best hit
                        }
                        for (int j = 0; j < 4 && walk; ++j) {
                            const int cell = trc_dda_cell(G, dd);
                            SB_COUNT(0, 1);
                            const bool any = ((occ[cell >> 5] >> (cell & 31)) & 1u) != 0u;
                            if (any) SB_COUNT(4, 1);
                            if (any) {
                                kc = G.off[cell]; kc1 = G.off[cell + 1];
                                n0 = ent[3 * (size_t)kc]; n1 = ent[3 * (size_t)kc + 1]; n2 = ent[3 * (size_t)kc + 2];
                            }
                            t_enter = fminf(dd.tnx, fminf(dd.tny, dd.tnz));
                            walk = trc_dda_next(G, r, tmax, &dd);
                            if (any) break;
                        }
                    }
                    // One exact test for every lane that has a candidate waiting, when a lane's list is full or half of the lanes
                    // have one: run whenever some lane had two, the exact tests took 25 turns per 64 rays for two tests per ray.
                    if (__ballot(nc >= CL_CAP) || __popcll(__ballot(nc > 0)) >= 32) SB_FLUSH_ROUND();
                }
            } else if (SB_FLAT_WALK) {
                unsigned kc = 0, kc1 = 0;
                while (__ballot(walk || kc < kc1)) {
                    if (kc < kc1) {
                        const unsigned sidx = G.list[kc];
                        ++kc;
                        if ((int)sidx != skip && trc_box_hit32(A.sbox + 6 * (size_t)sidx, r) &&
                            trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) SB_PUSH(sidx);
                    } else if (walk) {
                        if (sb != 0x7FFFFFFF) {
                            const float tbr = (float)(tb - t0);
                            if (tbr < t_enter - (1e-3f + 1e-4f * fabsf(tbr))) walk = false;    // every cell from here on starts behind the best hit
                        }
                        if (walk) {
                            const int cell = trc_dda_cell(G, dd);
                            kc = G.off[cell]; kc1 = G.off[cell + 1];
                            t_enter = fminf(dd.tnx, fminf(dd.tny, dd.tnz));
                            walk = trc_dda_next(G, r, tmax, &dd);
                        }
                    }
                    if (__ballot(nc >= CL_CAP - 1)) SB_FLUSH();
                }
            } else
            while (__ballot(walk)) {
                if (walk) {
                    if (sb != 0x7FFFFFFF) {
                        const float tbr = (float)(tb - t0);
                        if (tbr < t_enter - (1e-3f + 1e-4f * fabsf(tbr))) walk = false;    // every cell from here on starts behind the best hit
                    }
                }
                if (walk) {
                    const int cell = trc_dda_cell(G, dd);
                    const unsigned k1 = G.off[cell + 1];
                    for (unsigned k = G.off[cell]; k < k1; ++k) {
                        const unsigned sidx = G.list[k];
                        if ((int)sidx == skip) continue;      // the surface the ray stands on: no box test either
                        if (trc_box_hit32(A.sbox + 6 * (size_t)sidx, r) &&
                            trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) SB_PUSH(sidx);
                    }
                    t_enter = fminf(dd.tnx, fminf(dd.tny, dd.tnz));
                    walk = trc_dda_next(G, r, tmax, &dd);
                }
                if (__ballot(nc >= CL_CAP - 1)) SB_FLUSH();
            }
        } else if (walk) {
            for (int k = 0; k < sc.a_n_bleaf; ++k) {       // every bounded surface (accel = False: the reference's default)
                const unsigned sidx = sc.a_bleaf[k];
                if (trc_box_hit32(A.sbox + 6 * (size_t)sidx, r) &&
                    trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) SB_PUSH(sidx);
            }
        }
        SB_FLUSH();
#undef SB_FLUSH
#undef SB_FLUSH_ROUND
#undef SB_PUSH
#undef SB_TEST
        const bool hit = valid && tb < TRC_INF;
        if (FRESH) {            // a fresh ray that hits takes the next slot of the table
            const unsigned long long sl = chunk_append(&W.cnt[CN(CW_SLOTS)], cs, hit, nullptr, 0);
            if (hit) {
                if ((long long)sl < SQ_ROOM(W)) {
                    slot = (uint32_t)sl;
                    if (P.src) store_fresh_ray(W, slot, ri, px, py, pz, dx, dy, dz);
                    else store_fresh_ray(W, slot, ri, px, py, pz, dx, dy, dz, e0, ref0, wl0);
                } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
            }
        }
        bool listed = hit && slot != SQ_INVALID;
        if (split && absorb_here) {
            const bool term = listed && (sflags[sb] & TRC_SURF_TERMINAL) != 0;
            const unsigned long long tl = __ballot(term);
            if (tl) {
                double e = 0.0, hx = 0.0, hy = 0.0, hz = 0.0;
                int ts = -1;
                if (term) {
                    e = W.aux[slot].e;            // (a continued ray: its energy was written when it was shaded)
                    hx = px + tb * dx; hy = py + tb * dy; hz = pz + tb * dz;
                    ts = sb;
                    n_term += 1;
                }
                {   // the three sums: the lanes on the first lane's surface are summed in registers and added once (see k_s_absorb)
                    const int s0 = __shfl(ts, __ffsll((long long)tl) - 1, 64);
                    const bool in = term && ts == s0;
                    const double cnt = (double)__popcll(__ballot(in));
                    const double es = wave_sum(in ? e : 0.0);
                    if ((int)lane_id() == 0) { atomicAdd(&a_tally[s0], es); atomicAdd(&a_tally[Sn + s0], es); atomicAdd(&a_tally[2 * Sn + s0], cnt); }
                    if (term && !in) { atomicAdd(&a_tally[ts], e); atomicAdd(&a_tally[Sn + ts], e); atomicAdd(&a_tally[2 * Sn + ts], 1.0); }
                }
                if (term) record_hit<true>(La, a_tally, sb, e, e, hx, hy, hz, dx, dy, dz, P.capture != 0, left, &hc, a_fm, false, true);
                if (P.capture) chunk_rebroadcast(hc, __ffsll((long long)tl) - 1);
            }
            if (term) listed = false;
        } else if (split) {
            const bool term = listed && (sflags[sb] & TRC_SURF_TERMINAL) != 0;
            const unsigned long long q2 = chunk_append(&W.cnt[CN(CW_TERM_LIST)], ct, term, t_slot, SQ_ROOM(W));
            if (term) {
                if ((long long)q2 < SQ_ROOM(W)) { t_slot[q2] = slot; t_surf[q2] = (uint32_t)sb; t_t[q2] = tb; }
                else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
                listed = false;
            }
        }
        const unsigned long long q = chunk_append(&W.cnt[CN(CW_HIT_LIST)], ch, listed, W.hit_slot, SQ_ROOM(W));
        if (listed) {
            if ((long long)q < SQ_ROOM(W)) { W.hit_slot[q] = slot; W.hit_surf[q] = (uint32_t)sb; W.hit_t[q] = tb; }
            else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
        }
    }
    chunk_close(ch, W.hit_slot, SQ_ROOM(W));
    if (split && !absorb_here) chunk_close(ct, W.q1_slot, SQ_ROOM(W));
    if (absorb_here) {
        if (P.capture && wave_a < SHADE_MAX_WAVES && lane_id() == 0) hit_chunk_suspend(hc, W.hit_state + 2 * wave_a, S.hit_epoch);
        const double h = wave_sum((double)n_term);
        if (lane_id() == 0) atomicAdd(&a_tally[3 * Sn], h);
        __syncthreads();
        if (tid == 0) {
            const unsigned long long hh = (unsigned long long)(a_tally[3 * Sn] + 0.5);
            if (hh) { atomicAdd(&W.cnt[CN(CW_HITS)], hh); atomicAdd(&W.cnt[CN(CW_TERM_HITS)], hh); }
        }
        flush_sums<THREADS>(La0.tally, a_tally, 3 * Sn, a_fm, S.lds_fm_bins, Sn);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// k_s_bounce on the large grid with the tests of a wave's 64 rays shared out among its 64 lanes.  In k_s_bounce<2> a lane tests the
// faces listed for ITS ray's cells and runs ITS exact tests: on the relief of 105 800 triangles a wave took 33 / 84 turns of the
// walk (fresh / continued rays) where a lane needs 14 / 25, and 9 / 19 rounds of exact tests for two tests per ray -- two thirds of
// the vector instructions were lanes waiting for the slowest ray of their wave.  Here, per stage:
//   walk     every lane steps ITS ray through the grid (occupancy bits in LDS: nothing is read for an empty cell) until it has
//            SBC_CELLS cells that list something, and leaves their list ranges in LDS;
//   drain A  the listed faces of all those cells -- one list, in the order (lane, cell, entry) -- are tested 64 at a time, lane e
//            of a turn taking entry e: its owner by binary search in the prefix sums, the owner's single-precision ray by
//            wave shuffles, the face from its 48-byte list entry (consecutive lanes read consecutive entries).  What passes is a
//            (ray, surface) pair in the wave's queue;
//   drain B  64 pairs at a time get their exact float64 test, lane p taking pair p with the owner's ray by shuffles; the nearest
//            hit per ray is kept by LDS atomics -- the distance (positive doubles order like their bits), then, among the tests
//            that gave that distance, the lowest surface index: the reference's tie rule (tracer_engine.py:58-63);
// and a ray stops walking at the first cell that starts behind its nearest hit so far.  Same candidates (a superset is tested
// exactly where a ray's walk runs a stage ahead of its exact tests), same exact test, same results as k_s_bounce<2>.
// (SBC_CELLS, SBC_PAIRS and SBC_WAVE_BYTES, the wave's block of LDS, stand with the LDS layout in trc_bounds.h)
template <bool FRESH, bool FLAT, bool SUN = false>
__global__ __launch_bounds__(SB_THREADS) void k_s_bounce_coop(StreamParams S) {
    constexpr int THREADS = SB_THREADS;
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = S.P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    const int tid = threadIdx.x;
    const unsigned lane = lane_id();
    trc_accel_view A = stream_accel_global(sc, 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) A.root[i] = sc.a_bg_root[i];
    A.always = sc.a_bg_apart;
    A.n_always = sc.a_bg_napart;
    const double *recs = sc.recs;
    const float *obb = sc.a_obb;
    const int32_t *sflags = sc.sflags;
    trc_grid_view32 G;
    memset(&G, 0, sizeof(G));
    G.off = sc.a_bg_off; G.list = nullptr;
    G.nx = sc.a_bg_dim[0]; G.ny = sc.a_bg_dim[1]; G.nz = sc.a_bg_dim[2];
    G.lox = sc.a_bg_lo[0]; G.loy = sc.a_bg_lo[1]; G.loz = sc.a_bg_lo[2];
    G.csx = sc.a_bg_cs[0]; G.csy = sc.a_bg_cs[1]; G.csz = sc.a_bg_cs[2];
    G.ivx = sc.a_bg_inv[0]; G.ivy = sc.a_bg_inv[1]; G.ivz = sc.a_bg_inv[2];
    char *cur = (char *)lds;
    trc_buie_fast *l_bf = nullptr;
    if (FRESH) { l_bf = (trc_buie_fast *)cur; cur += (sizeof(trc_buie_fast) + 15) & ~(size_t)15; }
    const uint32_t *occ = sc.a_bg_occ;
    if (S.bg_occ_words > 0) {
        uint32_t *l_occ = (uint32_t *)cur; cur += (((size_t)S.bg_occ_words * 4) + 15) & ~(size_t)15;
        for (int i = tid; i < S.bg_occ_words; i += THREADS) l_occ[i] = sc.a_bg_occ[i];
        occ = l_occ;
    }
    // the wave's own LDS: list ranges of the collected cells, prefix sums, waiting pairs, nearest hit per ray
    char *wb = cur + (size_t)(tid >> 6) * SBC_WAVE_BYTES;
    uint32_t *c_off = (uint32_t *)wb; wb += SBC_CELLS * 64 * 4;         // [cell][lane]
    uint32_t *c_cnt = (uint32_t *)wb; wb += SBC_CELLS * 64 * 4;
    uint32_t *pre = (uint32_t *)wb; wb += 64 * 4;
    uint32_t *pairs = (uint32_t *)wb; wb += SBC_PAIRS * 4;              // owner lane | surface << 6
    unsigned long long *best_t = (unsigned long long *)wb; wb += 64 * 8;
    uint32_t *best_s = (uint32_t *)wb;
    const bool buie_src = FRESH && P.src && (P.src->kind == TRC_SRC_BUIE_DISK || P.src->kind == TRC_SRC_BUIE_RECT);
    if (FRESH) {
        if (buie_src) trc_buie_fast_fill(P.src->buie, l_bf, 0, tid, THREADS);
        __syncthreads();
        if (buie_src) trc_buie_fast_fill(P.src->buie, l_bf, 1, tid, THREADS);
    }
    __syncthreads();
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    const uint32_t *list = FRESH ? S.gen_list : S.act_in;
    long long count = FRESH ? (list ? (long long)W.cnt[CN(CW_GEN_LIST)] : S.nb) : (long long)W.cnt[CN(CW_ACT_IN)];
    if (list && count > (FRESH ? SQ_ROOM(W) : W.act_room)) count = FRESH ? SQ_ROOM(W) : W.act_room;
    const long long padded = (count + 63) & ~63ll;
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk ch = S.static_first ? (FRESH ? chunk_init_static_at(S.chunk_first, (unsigned long long)S.hit_base0 + wave_g * S.chunk_first) : chunk_init_static(S.chunk_hit, wave_g))
                                  : chunk_init(FRESH ? S.chunk_first : S.chunk_hit);
    WaveChunk cs = (FRESH && S.static_first) ? chunk_init_static_at(S.chunk_first, (unsigned long long)S.slot_base0 + wave_g * S.chunk_first) : chunk_init(S.chunk_first);
    const bool split = !FRESH && S.split_terminal;          // (1: behind a list, for k_s_absorb; the host does not ask for 2 here)
    WaveChunk ct = (split && S.static_first) ? chunk_init_static(S.chunk_thit, wave_g) : chunk_init(S.chunk_thit);
    uint32_t *const t_slot = W.q1_slot;
    uint32_t *const t_surf = (uint32_t *)W.q1_a;
    double *const t_t = (double *)W.q1_b;
    const float4 *ent = (const float4 *)sc.a_bg_ent;
    const bool wide_tri = sc.stride >= 20;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const unsigned long long T_INF_BITS = 0x7FF0000000000000ull;
    const long long bstride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += bstride) {
        uint32_t slot = SQ_INVALID, ri = SQ_INVALID;
        if (i < count) { if (FRESH) ri = list ? list[i] : (uint32_t)i; else slot = S.act_in[i]; }
        const bool valid = FRESH ? ri != SQ_INVALID : slot != SQ_INVALID;
        if (!__ballot(valid)) continue;
        if (valid) SB_COUNT(7, 1);
        if (lane == 0) SB_COUNT(9, 1);
        double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 1, e0 = 0, ref0 = 1.0, wl0 = 0.0;
        int skip = -1;
        if (valid) {
            if (FRESH) {
                unsigned long long rid;
                fast_new_ray<-1, false, SUN>(P, nullptr, S.base + ri, px, py, pz, dx, dy, dz, e0, ref0, wl0, rid, buie_src ? l_bf : nullptr);
            } else {
                const SRayGeo g = W.geo[slot];
                px = g.px; py = g.py; pz = g.pz; dx = g.dx; dy = g.dy; dz = g.dz;
                const uint32_t pw = (uint32_t)(g.tail >> 32);
                if (pw & SQ_SKIP_SELF) skip = (int)(pw & ~SQ_SKIP_SELF);
            }
        }
        best_t[lane] = T_INF_BITS;
        best_s[lane] = 0x7FFFFFFFu;
        double tb = TRC_INF;            // the lane's copy of its ray's nearest hit so far (best_t / best_s hold the truth)
        int sb = 0x7FFFFFFF;
        unsigned n_pairs = 0;           // (the same in every lane)
        // one round of exact tests: the last `take` pairs of the queue
        auto exact_round = [&]() __attribute__((always_inline)) {
            const unsigned take = n_pairs < 64u ? n_pairs : 64u;
            if (lane == 0) SB_COUNT(6, 1);
            const bool act = lane < take;
            const uint32_t pr = act ? pairs[n_pairs - take + lane] : 0u;
            const int owner = (int)(pr & 63u);
            const int sidx = (int)(pr >> 6);
            const double qx = __shfl(px, owner, 64), qy = __shfl(py, owner, 64), qz = __shfl(pz, owner, 64);
            const double ex = __shfl(dx, owner, 64), ey = __shfl(dy, owner, 64), ez = __shfl(dz, owner, 64);
            unsigned long long tbits = T_INF_BITS;
            if (act) {
                SB_COUNT(3, 1);
                const double *rec = recs + (size_t)sidx * sc.stride;
                double t;
                if (wide_tri) {         // the whole record of a triangular face in ten 16-byte loads (see k_s_bounce)
                    double l[20];
                    const double2 *q = (const double2 *)rec;
#pragma unroll
                    for (int k = 0; k < 10; ++k) { const double2 v = q[k]; l[2 * k] = v.x; l[2 * k + 1] = v.y; }
                    const int kind = trc_rec_gm_kind(l);
                    t = kind == TRC_GM_TRIANGLE ? trc_intersect_flat(TRC_GM_TRIANGLE, l, sc.extra, qx, qy, qz, ex, ey, ez)
                      : (FLAT ? trc_intersect_flat(kind, rec, sc.extra, qx, qy, qz, ex, ey, ez) : trc_intersect(rec, sc.extra, qx, qy, qz, ex, ey, ez));
                } else
                    t = FLAT ? trc_intersect_flat(trc_rec_gm_kind(rec), rec, sc.extra, qx, qy, qz, ex, ey, ez) : trc_intersect(rec, sc.extra, qx, qy, qz, ex, ey, ez);
                if (t > 0.0 && t < TRC_INF) { tbits = (unsigned long long)__double_as_longlong(t); atomicMin(&best_t[owner], tbits); }
            }
            WAVE_SYNC();
            {   // a ray whose nearest distance has just come down starts its choice of surface afresh
                const unsigned long long now = best_t[lane];
                if (now < (unsigned long long)__double_as_longlong(tb)) { tb = __longlong_as_double((long long)now); best_s[lane] = 0x7FFFFFFFu; }
            }
            WAVE_SYNC();
            if (act && tbits != T_INF_BITS && tbits == best_t[owner]) atomicMin(&best_s[owner], (uint32_t)sidx);
            WAVE_SYNC();
            sb = (int)best_s[lane];
            n_pairs -= take;
        };
        auto push_pair = [&](bool want, int owner, int sidx) __attribute__((always_inline)) {
            const unsigned long long m = __ballot(want);
            if (!m) return;
            if (want) pairs[n_pairs + (unsigned)__popcll(m & lanes_below)] = (uint32_t)owner | ((uint32_t)sidx << 6);
            n_pairs += (unsigned)__popcll(m);
            WAVE_SYNC();
            while (n_pairs > SBC_PAIRS - 64u) exact_round();        // (room for the next 64)
        };
        WAVE_SYNC();
        trc_ray32 r;
        memset(&r, 0, sizeof(r));
        double t0 = 0.0;
        bool walk = false;
        float tmin = 1.0f, tmax = 0.0f, t_enter = 0.0f;
        trc_dda dd;
        dd.cx = dd.cy = dd.cz = 0; dd.tnx = dd.tny = dd.tnz = 0.0f;
        {
            // surfaces without a box, then the few set apart from the grid (their boxes tested by the lane of the ray)
            for (int k = 0; k < A.n_unbounded; ++k) push_pair(valid && A.unbounded[k] != skip, (int)lane, A.unbounded[k]);
            const bool in = valid && trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0);
            for (int k = 0; k < A.n_always; ++k) {
                const int sidx = A.always[k];
                const float *b = A.sbox + 6 * (size_t)sidx;
                if (b[3] == TRC_INF && b[0] == -TRC_INF) continue;
                const bool want = in && sidx != skip && trc_box_hit32(b, r) && trc_obb_hit32(obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
                push_pair(want, (int)lane, sidx);
            }
            if (in) walk = trc_kd32_root(A.root, r, &tmin, &tmax);
            if (walk) { trc_dda_start(G, r, tmin, &dd); t_enter = tmin; }
        }
        for (;;) {
            // walk: up to SBC_CELLS cells of this lane's ray that list something
            unsigned cnt = 0, mine_total = 0;
            while (walk && cnt < SBC_CELLS) {
                if (sb != 0x7FFFFFFF) {
                    const float tbr = (float)(tb - t0);
                    if (tbr < t_enter - (1e-3f + 1e-4f * fabsf(tbr))) { walk = false; break; }     // every cell from here on starts behind the best hit
                }
                const int cell = trc_dda_cell(G, dd);
                SB_COUNT(0, 1);
                if ((occ[cell >> 5] >> (cell & 31)) & 1u) {
                    SB_COUNT(4, 1);
                    const uint32_t o0 = G.off[cell], o1 = G.off[cell + 1];
                    c_off[cnt * 64 + lane] = o0; c_cnt[cnt * 64 + lane] = o1 - o0;
                    mine_total += o1 - o0;
                    ++cnt;
                }
                t_enter = fminf(dd.tnx, fminf(dd.tny, dd.tnz));
                walk = trc_dda_next(G, r, tmax, &dd);
            }
            // drain A: all listed faces of the collected cells, 64 per turn
            unsigned incl = mine_total;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(incl, off, 64);
                if ((int)lane >= off) incl += o;
            }
            const unsigned total = __shfl(incl, 63, 64);
            pre[lane] = incl;
            for (unsigned k = cnt; k < SBC_CELLS; ++k) c_cnt[k * 64 + lane] = 0u;
            WAVE_SYNC();
            for (unsigned base = 0; base < total; base += 64) {
                if (lane == 0) SB_COUNT(5, 1);
                const unsigned e = base + lane;
                const bool ev = e < total;
                int owner = 0;
                uint32_t at = 0;
                if (ev) {
                    SB_COUNT(1, 1);
                    unsigned lo = 0, hi = 63;
                    while (lo < hi) {
                        const unsigned mid = (lo + hi) >> 1;
                        if (pre[mid] > e) hi = mid; else lo = mid + 1;
                    }
                    owner = (int)lo;
                    unsigned j = e - (owner ? pre[owner - 1] : 0u);
#pragma unroll
                    for (int k = 0; k < SBC_CELLS; ++k) {
                        const unsigned c = c_cnt[k * 64 + owner];
                        if (j < c) { at = c_off[k * 64 + owner] + j; j = 0xFFFFFFFFu; }
                        else if (j != 0xFFFFFFFFu) j -= c;
                    }
                }
                trc_ray32 ro;
                ro.ox = __shfl(r.ox, owner, 64); ro.oy = __shfl(r.oy, owner, 64); ro.oz = __shfl(r.oz, owner, 64);
                ro.dx = __shfl(r.dx, owner, 64); ro.dy = __shfl(r.dy, owner, 64); ro.dz = __shfl(r.dz, owner, 64);
                ro.ix = __shfl(r.ix, owner, 64); ro.iy = __shfl(r.iy, owner, 64); ro.iz = __shfl(r.iz, owner, 64);
                const int skip_o = __shfl(skip, owner, 64);
                bool pass = false;
                int sidx = 0;
                if (ev) {
                    const float4 c0 = ent[3 * (size_t)at], c1 = ent[3 * (size_t)at + 1], c2 = ent[3 * (size_t)at + 2];
                    const uint32_t w = __float_as_uint(c0.x);
                    sidx = (int)(w & 0x7FFFFFFFu);
                    if (sidx != skip_o) {
                        if (!(w & 0x80000000u)) pass = trc_tri_hit32(c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, A.delta, ro);
                        else {
                            const float b[6] = {c0.y, c0.z, c0.w, c1.x, c1.y, c1.z};
                            pass = trc_box_hit32(b, ro) && trc_obb_hit32(obb + (size_t)TRC_OBB_STRIDE * sidx, ro.ox, ro.oy, ro.oz, ro.dx, ro.dy, ro.dz);
                        }
                    }
                    if (pass) SB_COUNT(2, 1);
                }
                push_pair(pass, owner, sidx);
            }
            WAVE_SYNC();
            // drain B: full rounds while the walk goes on, everything once it is over
            const bool walking = __ballot(walk) != 0ull;
            while (n_pairs >= 64u || (!walking && n_pairs > 0u)) exact_round();
            if (!walking) break;
        }
        const bool hit = valid && sb != 0x7FFFFFFF && tb < TRC_INF;
        if (FRESH) {            // a fresh ray that hits takes the next slot of the table
            const unsigned long long sl = chunk_append(&W.cnt[CN(CW_SLOTS)], cs, hit, nullptr, 0);
            if (hit) {
                if ((long long)sl < SQ_ROOM(W)) {
                    slot = (uint32_t)sl;
                    SRayGeo g;
                    g.px = px; g.py = py; g.pz = pz; g.dx = dx; g.dy = dy; g.dz = dz;
                    g.head = SQ_INVALID;
                    g.idx = ri;
                    g.tail = sray_tail(0, 0u);
                    W.geo[slot] = g;
                    if (!P.src) {
                        SRayAux a;
                        a.e = e0; a.ref = ref0; a.wl = wl0; a.pad = 0.0;
                        W.aux[slot] = a;
                    }
                } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
            }
        }
        bool listed = hit && slot != SQ_INVALID;
        if (split) {
            const bool term = listed && (sflags[sb] & TRC_SURF_TERMINAL) != 0;
            const unsigned long long q2 = chunk_append(&W.cnt[CN(CW_TERM_LIST)], ct, term, t_slot, SQ_ROOM(W));
            if (term) {
                if ((long long)q2 < SQ_ROOM(W)) { t_slot[q2] = slot; t_surf[q2] = (uint32_t)sb; t_t[q2] = tb; }
                else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
                listed = false;
            }
        }
        const unsigned long long q = chunk_append(&W.cnt[CN(CW_HIT_LIST)], ch, listed, W.hit_slot, SQ_ROOM(W));
        if (listed) {
            if ((long long)q < SQ_ROOM(W)) { W.hit_slot[q] = slot; W.hit_surf[q] = (uint32_t)sb; W.hit_t[q] = tb; }
            else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
        }
    }
    chunk_close(ch, W.hit_slot, SQ_ROOM(W));
    if (split) chunk_close(ct, t_slot, SQ_ROOM(W));
}

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_s_exact(StreamParams S) {
    extern __shared__ double lds[];
    const DScene &sc = S.P.sc;
    const StreamWs &W = S.W;
    // surface records in LDS when they fit (S.lds_recs): the per-lane gathers of 17 doubles leave the memory pipeline
    const double *recs = sc.recs;
    if (S.lds_recs) {
        for (int i = threadIdx.x; i < sc.n_surf * sc.stride; i += blockDim.x) lds[i] = sc.recs[i];
        __syncthreads();
        recs = lds;
    }
    if (W.cnt[CN(CW_OVERFLOW)]) return;       // the candidate queue overflowed in k_s_walk: nothing of this bounce is committed, the host retries
    long long n3 = (long long)W.cnt[CN(CW_Q3)];
    if (n3 > W.q3_cap) n3 = W.q3_cap;
    const long long padded = (n3 + 63) & ~63ll;
    WaveChunk ch = S.static_general ? chunk_init_static_at(SQ_CHUNK, (unsigned long long)S.hit_base0 + (((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * SQ_CHUNK) : chunk_init();
    const long long stride = (long long)gridDim.x * blockDim.x;
    // two entries per lane and iteration: their gathers and atomics are in flight together (the kernel is bound by the
    // round trips ray record -> exact test -> atomicMin, not by arithmetic)
    for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < padded; i0 += 2 * stride) {
        const long long i1 = i0 + stride;
        uint32_t slot0 = SQ_INVALID, slot1 = SQ_INVALID, sidx0 = 0, sidx1 = 0;
        if (i0 < n3) { slot0 = W.q3_slot[i0]; sidx0 = W.q3_surf[i0]; }
        if (i1 < n3) { slot1 = W.q3_slot[i1]; sidx1 = W.q3_surf[i1]; }
        SRayGeo g0, g1;
        g0.px = g0.py = g0.pz = g0.dx = g0.dy = 0.0; g0.dz = 1.0;
        g1 = g0;
        if (slot0 != SQ_INVALID) g0 = W.geo[slot0];
        if (slot1 != SQ_INVALID) g1 = W.geo[slot1];
        double t0 = TRC_INF, t1 = TRC_INF;
        if (slot0 != SQ_INVALID) {
            t0 = trc_intersect(recs + (size_t)sidx0 * sc.stride, sc.extra, g0.px, g0.py, g0.pz, g0.dx, g0.dy, g0.dz);
            if (!(t0 > 0.0) || !(t0 < TRC_INF)) t0 = TRC_INF;      // t == 0 is not a hit (tracer_engine.py:58)
        }
        if (slot1 != SQ_INVALID) {
            t1 = trc_intersect(recs + (size_t)sidx1 * sc.stride, sc.extra, g1.px, g1.py, g1.pz, g1.dx, g1.dy, g1.dz);
            if (!(t1 > 0.0) || !(t1 < TRC_INF)) t1 = TRC_INF;
        }
        // a finite t links the entry into its ray's list (the newest entry is the head); the entry that finds the list empty
        // also enters the ray in the hit list -- exactly once per ray
        uint32_t prev0 = 0, prev1 = 0;
        if (t0 < TRC_INF) prev0 = atomicExch(&W.geo[slot0].head, (uint32_t)i0);
        if (t1 < TRC_INF) prev1 = atomicExch(&W.geo[slot1].head, (uint32_t)i1);
        if (t0 < TRC_INF) { SCand c; c.t = t0; c.surf = sidx0; c.next = prev0; W.q3n[i0] = c; }
        if (t1 < TRC_INF) { SCand c; c.t = t1; c.surf = sidx1; c.next = prev1; W.q3n[i1] = c; }
        const bool first0 = t0 < TRC_INF && prev0 == SQ_INVALID, first1 = t1 < TRC_INF && prev1 == SQ_INVALID;
        unsigned long long q = chunk_append(&W.cnt[CN(CW_HIT_LIST)], ch, first0, W.hit_slot, SQ_ROOM(W));
        if (first0) { if ((long long)q < SQ_ROOM(W)) { W.hit_slot[q] = slot0; W.hit_surf[q] = SQ_INVALID; } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; }
        q = chunk_append(&W.cnt[CN(CW_HIT_LIST)], ch, first1, W.hit_slot, SQ_ROOM(W));
        if (first1) { if ((long long)q < SQ_ROOM(W)) { W.hit_slot[q] = slot1; W.hit_surf[q] = SQ_INVALID; } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; }
    }
    chunk_close(ch, W.hit_slot, SQ_ROOM(W));
}

// The hit list of a bounce parted by optics class, for scenes with more than one shading kernel: the lanes of a wave of the
// cavity's hit list sit on a mirror, on diffuse walls and on a conductor, and every class kernel would walk the whole list
// with a part of its lanes at work.  One lane per entry: surface and distance resolved (general path: the nearest of the ray's
// linked candidates, lowest surface index on equal t, tracer_engine.py:58-63), class looked up, entry appended to its class's
// list -- 16 bytes read, 16 written per hit.
__global__ __launch_bounds__(256) void k_s_partition(StreamParams S) {
    const DScene &sc = S.P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    long long nh = (long long)W.cnt[CN(CW_HIT_LIST)];
    if (nh > SQ_ROOM(W)) nh = SQ_ROOM(W);
    const long long padded = (nh + 63) & ~63ll;
    const unsigned long long wave_g = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk pc[TRC_CLS_COUNT];
#pragma unroll
    for (int c = 0; c < TRC_CLS_COUNT; ++c)
        pc[c] = S.part_static[c] ? chunk_init_static_at(S.part_chunk[c], wave_g * S.part_chunk[c]) : chunk_init(S.part_chunk[c]);
    // four entries per lane and turn: their loads -- entry, then the flags of its surface (and the candidates of a general-path entry) --
    // are in flight together; one entry per turn left the kernel waiting 90 % of its wave cycles
    const long long pstride = (long long)gridDim.x * blockDim.x;
    for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < padded; i0 += 4 * pstride) {
        uint32_t slot[4], hs[4];
        double t[4];
        int cls[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + u * pstride;
            slot[u] = SQ_INVALID; hs[u] = SQ_INVALID; t[u] = TRC_INF; cls[u] = -1;
            if (i < nh) { slot[u] = W.hit_slot[i]; hs[u] = W.hit_surf[i]; t[u] = W.hit_t[i]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (slot[u] != SQ_INVALID) {
                if (hs[u] == SQ_INVALID) {
                    double tt = TRC_INF;
                    int sb = 0x7FFFFFFF;
                    nearest_linked(W.q3n, W.geo[slot[u]].head, tt, sb);
                    hs[u] = (uint32_t)sb; t[u] = tt;
                }
                if (hs[u] < (uint32_t)Sn) {
                    const int fl = sc.sflags[hs[u]];
                    cls[u] = (S.shade_term_cls >= 0 && (fl & TRC_SURF_TERMINAL)) ? S.shade_term_cls : ((fl >> TRC_SURF_CLS_SHIFT) & TRC_SURF_CLS_MASK);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!__ballot(cls[u] >= 0)) continue;
#pragma unroll
            for (int c = 0; c < TRC_CLS_COUNT; ++c) {
                if (!W.pl_slot[c]) continue;
                const unsigned long long q = chunk_append(&W.cnt[CN(CW_CLS_LIST + c)], pc[c], cls[u] == c, W.pl_slot[c], W.pl_room);
                if (cls[u] == c) {
                    if ((long long)q < W.pl_room) { W.pl_slot[c][q] = slot[u]; W.pl_surf[c][q] = hs[u]; W.pl_t[c][q] = t[u]; }
                    else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < TRC_CLS_COUNT; ++c)
        if (W.pl_slot[c]) chunk_close(pc[c], W.pl_slot[c], W.pl_room);
}

// WAVES: waves per SIMD the instance is built for, two workgroups of 128 * WAVES threads per CU (they share their LDS tables)
// LDS: tallies, records, optics parameters, flux-map tables, flags and table values are all staged in LDS -- or none of them is (as
// in k_s_fresh): a pointer that may be either is read with flat loads, and a flat load waits for every load in flight -- the ray
// records fetched ahead included (81 flat operations, 60 full waits in the instance that chose at run time).
// CHART: the flux maps may bin in the charts other than XY (record_hit, trc_device.h)
template <bool SIMPLE, int WAVES, bool LDS, bool SPEC = false, bool CHART = false>
__global__ __launch_bounds__(128 * WAVES, WAVES) void k_s_shade(StreamParams S) {
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    // LDS: tallies | surface records | optics parameters | flux-map tables and capture flags.  Everything a hit looks up by
    // surface index is read from LDS: from global memory each of them is a dependent round trip (the flux-map bin search
    // alone was twelve of them per hit).
    // (the image of TRC_IMG_SHADE, trc_shade_lds_layout in trc_bounds.h, by which the host sizes the launch: carved here in its order --
    // this kernel sits at its register limit, and through a shared staging routine five of its instances spilled more scalar registers)
    FastParams Pl = S.P;
    Pl.sc.tally = W.tally_part + (size_t)(blockIdx.x % TALLY_PARTS) * (size_t)W.tally_n;
    double *l_tally = lds;
    double *cur = lds + (LDS ? 3 * Sn + 2 : 1);
    if (LDS) for (int i = threadIdx.x; i < 3 * Sn + 2; i += blockDim.x) l_tally[i] = 0.0;
    const double *recs = sc.recs;
    if (LDS) {
        double *l_recs = cur; cur += Sn * sc.stride;
        for (int i = threadIdx.x; i < Sn * sc.stride; i += blockDim.x) l_recs[i] = sc.recs[i];
        recs = l_recs;
        double *l_opt = cur; cur += 8 * Sn;
        for (int i = threadIdx.x; i < 8 * Sn; i += blockDim.x) l_opt[i] = sc.opt[i];
        double *l_edges = cur; cur += sc.n_fm_edges;
        for (int i = threadIdx.x; i < sc.n_fm_edges; i += blockDim.x) l_edges[i] = sc.fm_edges[i];
        FluxMapDev *l_fms = (FluxMapDev *)cur; cur += (sc.n_fm * sizeof(FluxMapDev) + 7) / 8;
        for (int i = threadIdx.x; i < sc.n_fm; i += blockDim.x) l_fms[i] = sc.fms[i];
        int32_t *l_fm_of = (int32_t *)cur;
        int32_t *l_flags = l_fm_of + Sn;
        for (int i = threadIdx.x; i < Sn; i += blockDim.x) { l_fm_of[i] = sc.fm_of_surf ? sc.fm_of_surf[i] : -1; l_flags[i] = sc.sflags[i]; }
        Pl.sc.opt = l_opt; Pl.sc.fm_edges = l_edges; Pl.sc.fms = l_fms; Pl.sc.fm_of_surf = l_fm_of; Pl.sc.sflags = l_flags;
        cur = (double *)(((uintptr_t)(l_flags + Sn) + 7) & ~(uintptr_t)7);
        double *l_extra = cur; cur += sc.n_extra;          // (optics tables: absorptance over angle / wavelength, complex indices)
        for (int i = threadIdx.x; i < sc.n_extra; i += blockDim.x) l_extra[i] = sc.extra[i];
        Pl.sc.extra = l_extra;
    }
    double *l_fm = nullptr;         // private copy of the flux-map bins (S.lds_fm_bins of them)
    if (S.lds_fm_bins > 0) {
        l_fm = cur; cur += S.lds_fm_bins;
        for (int i = threadIdx.x; i < S.lds_fm_bins; i += blockDim.x) l_fm[i] = 0.0;
    }
    const double src_energy = P.src ? P.src->energy : 0.0;
    __syncthreads();
    long long nh = (long long)W.cnt[S.hl_cn];
    if (nh > S.hl_room) nh = S.hl_room;     // never read beyond the allocation, whatever the counter says
    const long long padded = (nh + 63) & ~63ll;
    WaveChunk ca = S.static_first ? chunk_init_static_at(S.chunk_act, (unsigned long long)S.act_base0 + (((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * S.chunk_act)
                                  : chunk_init(S.chunk_act);
    // this wave's open chunk of the scene's hit buffer, carried over from earlier launches: entries are only left unused
    // in the chunks open when the buffer is read (they keep the surface index -1 the buffer is cleared with)
    const unsigned wave_g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk hc = chunk_init(S.chunk_hitbuf);
    if (P.capture && wave_g < SHADE_MAX_WAVES) hit_chunk_resume(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    unsigned n_hit = 0, n_alive = 0;
    // Two loads stand in front of every hit -- its entry of the hit list, then the ray record the entry points to -- and at 2 waves
    // per SIMD nothing hides them.  Both are fetched ahead, in two stages: while hit i is worked on, the record of hit i + 1 (whose
    // entry arrived an iteration ago) and the entry of hit i + 2 are on their way.
    const long long stride = (long long)gridDim.x * blockDim.x;
    uint32_t slot_a = SQ_INVALID, hs_a = SQ_INVALID;       // stage A: entry of the hit after the next
    double ht_a = 0.0;
    uint32_t slot_n = SQ_INVALID, hs_n = SQ_INVALID;       // stage B: entry of the next hit ...
    double ht_n = 0.0;
    SRayGeo g_n;                                            // ... and the ray record behind it
    g_n.px = g_n.py = g_n.pz = g_n.dx = g_n.dy = 0.0; g_n.dz = 1.0; g_n.head = SQ_INVALID; g_n.idx = 0u; g_n.tail = 0ull;
    double ae_n = 0.0, ar_n = 1.0, aw_n = 0.0;     // ... and energy, index, wavelength (fresh rays of a source carry none: not read)
    const bool aux_always = !P.src;
    {
        const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i0 < nh) { slot_n = S.hl_slot[i0]; hs_n = S.hl_surf[i0]; ht_n = S.hl_t[i0]; }
        if (i0 + stride < nh) { slot_a = S.hl_slot[i0 + stride]; hs_a = S.hl_surf[i0 + stride]; ht_a = S.hl_t[i0 + stride]; }
        if (slot_n != SQ_INVALID) {
            g_n = W.geo[slot_n];
            if (aux_always || S.bounce_no > 0) { const SRayAux a = W.aux[slot_n]; ae_n = a.e; ar_n = a.ref; aw_n = a.wl; }
        }
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        bool alive = false;
        uint32_t slot = slot_n;
        uint32_t hs = hs_n;                                   // SQ_INVALID: the nearest of the ray's linked candidates is picked here
        double ht = ht_n;
        SRayGeo g = g_n;
        double ae = ae_n, ar = ar_n, aw = aw_n;
        // Everything fetched for this hit is made to arrive HERE, before the loads for the next ones are issued: the compiler places
        // its wait in front of the first use of a loaded register, and across the loop's back edge it only knows "something is in
        // flight" -- that wait, vmcnt(0), would otherwise sit in the middle of the body and take the fresh loads with it.
        asm volatile("" : "+v"(slot), "+v"(hs), "+v"(ht), "+v"(slot_a), "+v"(hs_a), "+v"(ht_a));
        asm volatile("" : "+v"(g.px), "+v"(g.py), "+v"(g.pz), "+v"(g.dx), "+v"(g.dy), "+v"(g.dz), "+v"(g.head), "+v"(g.idx), "+v"(g.tail));
        asm volatile("" : "+v"(ae), "+v"(ar), "+v"(aw));
        {
            slot_n = slot_a; hs_n = hs_a; ht_n = ht_a;
            if (slot_n != SQ_INVALID) {
                g_n = W.geo[slot_n];
                if (aux_always || S.bounce_no > 0) { const SRayAux a = W.aux[slot_n]; ae_n = a.e; ar_n = a.ref; aw_n = a.wl; }
            }
            const long long i2 = i + 2 * stride;
            slot_a = SQ_INVALID; hs_a = SQ_INVALID; ht_a = 0.0;
            if (i2 < nh) { slot_a = S.hl_slot[i2]; hs_a = S.hl_surf[i2]; ht_a = S.hl_t[i2]; }
        }
        bool has_hit = slot != SQ_INVALID;
        // nearest of the ray's linked hits; on equal t the lowest surface index (tracer_engine.py:58-63)
        double t = TRC_INF;
        int s = 0x7FFFFFFF;
        if (has_hit) {
            if (hs != SQ_INVALID) { t = ht; s = (int)hs; }
            else nearest_linked(W.q3n, g.head, t, s);
            // the hits on surfaces of the other optics classes are taken by their own kernels (trc_shade.hip)
            if ((unsigned)s < (unsigned)Sn) {
                const int fl = Pl.sc.sflags[s];
                const int cls = (fl >> TRC_SURF_CLS_SHIFT) & TRC_SURF_CLS_MASK;
                if (S.shade_cls >= 0)         // (< 0: this launch is the only shading kernel of the bounce)
                    has_hit = (S.shade_term_cls >= 0 && (fl & TRC_SURF_TERMINAL)) ? (S.shade_term_cls == S.shade_cls) : (cls == S.shade_cls);
            } else has_hit = false;
        }
        const unsigned long long hit_lanes = __ballot(has_hit);
        if (!hit_lanes) continue;            // the unused tail of a chunk of the list, or hits of other classes only
        int ts = -1;                         // the surface this lane's hit is tallied on, with absorbed and incident energy
        double tea = 0.0, tei = 0.0;
        if (has_hit) {
            n_hit += 1;
            double px = g.px, py = g.py, pz = g.pz, dx = g.dx, dy = g.dy, dz = g.dz;
            int bounce = (int)(uint32_t)g.tail;
            int prev = bounce == 0 ? Sn : (int)((uint32_t)(g.tail >> 32) & ~SQ_SKIP_SELF);      // the surface the ray left (transfer matrix); Sn = the source
            double e, ref, wl;
            const long long ray_no = S.base + (long long)g.idx;
            unsigned long long rid = P.rid ? P.rid[ray_no] : (P.ray_offset + (unsigned long long)ray_no);
            if (bounce == 0 && P.src) {
                e = src_energy;
                // a source with a spectrum: the wavelength is drawn here, at the ray's first hit (culled rays and misses never draw)
                if (SPEC) trc_spectrum_of(P.spec, P.seed, rid, &wl, &ref);
                else { ref = 1.0; wl = 0.0; }
            }
            else { e = ae; ref = ar; wl = aw; }
            const double e_in = e;
            bool vol = false;
            if (LDS) alive = fast_shade<true, SIMPLE, CHART>(Pl, recs, l_tally, t, s, px, py, pz, dx, dy, dz, e, ref, wl, rid, bounce, prev, &hc, l_fm, true, &vol);
            else alive = fast_shade<false, SIMPLE, CHART>(Pl, recs, l_tally, t, s, px, py, pz, dx, dy, dz, e, ref, wl, rid, bounce, prev, &hc, l_fm);
            if (LDS && !vol) { ts = s; tea = e_in - e; tei = e_in; }      // (a volume event tallies nothing)
            if (alive) {
                SRayGeo go;
                go.px = px; go.py = py; go.pz = pz; go.dx = dx; go.dy = dy; go.dz = dz;
                go.head = SQ_INVALID;          // ready for the next bounce's search
                go.idx = g.idx;
                // (a ray scattered in the medium before its first surface still has the source behind it: prev == Sn)
                uint32_t pw = (uint32_t)prev;
                if (prev < Sn && leaves_flat(recs + (size_t)prev * sc.stride, px, py, pz, dx, dy, dz)) pw |= SQ_SKIP_SELF;
                go.tail = sray_tail(bounce, pw);
                W.geo[slot] = go;
                SRayAux ao;
                ao.e = e; ao.ref = ref; ao.wl = wl; ao.pad = 0.0;
                W.aux[slot] = ao;
            }
        }
        if (LDS) {
            // The three sums per surface.  64 lanes adding to one word of LDS take 64 turns, and scenes of few surfaces (a dish
            // and its receiver, a cavity of seven walls) put most lanes of a wave on the same ones: while at least 8 lanes share
            // the surface of the first lane still to be served, they are summed in registers and added once; the others add for
            // themselves.  (tally_by_wave, trc_device.h, in this kernel's own text: through the helper two instances spilled more scalar
            // registers)
            unsigned long long todo = Sn <= 64 ? __ballot(ts >= 0) : 0ull;       // (a field of hundreds of mirrors: no lanes to share with)
            for (int round = 0; round < 6 && todo; ++round) {
                const int s0 = __shfl(ts, __ffsll((long long)todo) - 1, 64);
                const bool in = ts == s0;
                const unsigned long long m = __ballot(in);
                if (__popcll(m) < 8) break;
                const double a = wave_sum(in ? tea : 0.0), b = wave_sum(in ? tei : 0.0);
                if (lane_id() == 0) { atomicAdd(&l_tally[s0], a); atomicAdd(&l_tally[Sn + s0], b); atomicAdd(&l_tally[2 * Sn + s0], (double)__popcll(m)); }
                if (in) ts = -1;
                todo &= ~m;
            }
            if (ts >= 0) { atomicAdd(&l_tally[ts], tea); atomicAdd(&l_tally[Sn + ts], tei); atomicAdd(&l_tally[2 * Sn + ts], 1.0); }
        }
        if (hit_lanes && P.capture) chunk_rebroadcast(hc, __ffsll((long long)hit_lanes) - 1);   // hc was advanced by the lanes with a hit only
        unsigned long long q = chunk_append(&W.cnt[CN(CW_ACT_OUT)], ca, alive, S.act_out, W.act_room);
        if (alive) { if ((long long)q < W.act_room) S.act_out[q] = slot; else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; n_alive += 1; }
    }
    chunk_close(ca, S.act_out, W.act_room);
    if (P.capture && wave_g < SHADE_MAX_WAVES && lane_id() == 0) hit_chunk_suspend(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    // real (unpadded) counts of this bounce: hits and rays that go on -- one pair of atomics per workgroup where the tallies are in
    // LDS (flush_counts), per wave otherwise: its image has one word there that nobody reads.  (The bins are flushed with the tallies:
    // they are in LDS only when the tables are -- trc_shade_lds_choose -- so the instances without have none to flush.)
    if (LDS) {
        flush_counts<false>(l_tally + 3 * Sn, n_hit, n_alive, &W.cnt[CN(CW_HITS)], &W.cnt[CN(CW_CLS_HITS + TRC_CLS_GENERAL)], &W.cnt[CN(CW_ALIVE)]);
        flush_sums(Pl.sc.tally, l_tally, 3 * Sn, l_fm, S.lds_fm_bins, Sn);
    } else {
        const double h = wave_sum((double)n_hit), a = wave_sum((double)n_alive);
        if (lane_id() == 0) {
            atomicAdd(&W.cnt[CN(CW_HITS)], (unsigned long long)(h + 0.5)); atomicAdd(&W.cnt[CN(CW_ALIVE)], (unsigned long long)(a + 0.5));
            atomicAdd(&W.cnt[CN(CW_CLS_HITS + TRC_CLS_GENERAL)], (unsigned long long)(h + 0.5));
        }
    }
}

// The hits that k_s_bounce found on surfaces that end every ray (TRC_SURF_TERMINAL: the receiver of a field).  Nothing is drawn and
// nothing goes on: hit point, tallies, flux-map bin, hit capture.  A quarter of k_s_shade's registers, so eight waves per SIMD hide
// the two loads in front of every hit; k_s_shade at two could not (0.20 -> ms of an NSTTF batch's second bounce).
// LDS: tallies | flux-map edges, descriptors, surface -> map, flags | flux-map bins -- as k_s_shade with lds_tally, lds_tables.
__global__ __launch_bounds__(SA_THREADS, 2) void k_s_absorb(StreamParams S) {
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    // (the image of TRC_IMG_ABSORB, trc_shade_lds_layout in trc_bounds.h, by which the host sizes the launch: carved here in its order --
    // through a shared staging routine the kernel took six more scalar registers, one wave per SIMD of its eight)
    DScene L = sc;
    L.tally = W.tally_part + (size_t)(blockIdx.x % TALLY_PARTS) * (size_t)W.tally_n;
    double *l_tally = lds;
    double *cur = lds + 3 * Sn + 2;
    for (int i = threadIdx.x; i < 3 * Sn + 2; i += blockDim.x) l_tally[i] = 0.0;
    double *l_edges = cur; cur += sc.n_fm_edges;
    for (int i = threadIdx.x; i < sc.n_fm_edges; i += blockDim.x) l_edges[i] = sc.fm_edges[i];
    FluxMapDev *l_fms = (FluxMapDev *)cur; cur += (sc.n_fm * sizeof(FluxMapDev) + 7) / 8;
    for (int i = threadIdx.x; i < sc.n_fm; i += blockDim.x) l_fms[i] = sc.fms[i];
    int32_t *l_fm_of = (int32_t *)cur;
    int32_t *l_flags = l_fm_of + Sn;
    for (int i = threadIdx.x; i < Sn; i += blockDim.x) { l_fm_of[i] = sc.fm_of_surf ? sc.fm_of_surf[i] : -1; l_flags[i] = sc.sflags[i]; }
    L.fm_edges = l_edges; L.fms = l_fms; L.fm_of_surf = l_fm_of; L.sflags = l_flags;
    cur = (double *)(((uintptr_t)(l_flags + Sn) + 7) & ~(uintptr_t)7);
    double *l_fm = nullptr;
    if (S.lds_fm_bins > 0) {
        l_fm = cur;
        for (int i = threadIdx.x; i < S.lds_fm_bins; i += blockDim.x) l_fm[i] = 0.0;
    }
    const double src_energy = P.src ? P.src->energy : 0.0;
    __syncthreads();
    const uint32_t *t_slot = W.q1_slot;
    const uint32_t *t_surf = (const uint32_t *)W.q1_a;
    const double *t_t = (const double *)W.q1_b;
    long long nh = (long long)W.cnt[CN(CW_TERM_LIST)];
    if (nh > SQ_ROOM(W)) nh = SQ_ROOM(W);
    const long long padded = (nh + 63) & ~63ll;
    // this wave's open chunk of the scene's hit buffer: the second half of the state array (k_s_shade's waves own the first)
    const unsigned wave_g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk hc = chunk_init(S.chunk_hitbuf);
    if (P.capture && wave_g < SHADE_MAX_WAVES) hit_chunk_resume(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    unsigned n_hit = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t slot = i < nh ? t_slot[i] : SQ_INVALID;
        const bool has_hit = slot != SQ_INVALID;
        const unsigned long long hit_lanes = __ballot(has_hit);
        if (!hit_lanes) continue;
        int s = -1, prev = Sn;
        double e = 0.0, hx = 0.0, hy = 0.0, hz = 0.0, dx = 0.0, dy = 0.0, dz = 1.0;
        if (has_hit) {
            s = (int)t_surf[i];
            const double t = t_t[i];
            const SRayGeo g = W.geo[slot];
            const int bounce = (int)(uint32_t)g.tail;
            prev = bounce == 0 ? Sn : (int)((uint32_t)(g.tail >> 32) & ~SQ_SKIP_SELF);
            e = (bounce == 0 && P.src) ? src_energy : W.aux[slot].e;
            hx = g.px + t * g.dx; hy = g.py + t * g.dy; hz = g.pz + t * g.dz;
            dx = g.dx; dy = g.dy; dz = g.dz;
            n_hit += 1;
        }
        // The three sums of the surface: the hits of a wave are mostly on one surface (the receiver), and 64 lanes adding to one
        // word of LDS take 64 turns -- with 16 waves at it, that was the kernel.  The lanes on the first lane's surface are summed
        // in registers and added once; the others add for themselves.
        {
            const int leader = __ffsll((long long)hit_lanes) - 1;
            const int s0 = __shfl(s, leader, 64);
            const bool in = has_hit && s == s0;
            const double cnt = (double)__popcll(__ballot(in));
            const double es = wave_sum(in ? e : 0.0);
            if ((int)lane_id() == 0) {          // (wave_sum leaves the total in lane 0)
                atomicAdd(&l_tally[s0], es); atomicAdd(&l_tally[Sn + s0], es); atomicAdd(&l_tally[2 * Sn + s0], cnt);
            }
            if (has_hit && !in) { atomicAdd(&l_tally[s], e); atomicAdd(&l_tally[Sn + s], e); atomicAdd(&l_tally[2 * Sn + s], 1.0); }
        }
        if (has_hit) record_hit<true>(L, l_tally, s, e, e, hx, hy, hz, dx, dy, dz, P.capture != 0, prev, &hc, l_fm, false, true);
        if (P.capture) chunk_rebroadcast(hc, __ffsll((long long)hit_lanes) - 1);
    }
    if (P.capture && wave_g < SHADE_MAX_WAVES && lane_id() == 0) hit_chunk_suspend(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    // (CN(CW_TERM_HITS): the host sizes the two lists of the batches to come by their shares)
    flush_counts<false>(l_tally + 3 * Sn, n_hit, 0u, &W.cnt[CN(CW_HITS)], &W.cnt[CN(CW_TERM_HITS)], nullptr);
    flush_sums(L.tally, l_tally, 3 * Sn, l_fm, S.lds_fm_bins, Sn);
}

// adds the private copies of one slot into the scene's tally buffer and clears them
__global__ void k_s_merge_tallies(double *tally, double *parts, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int k = 0; k < TALLY_PARTS; ++k) { sum += parts[(size_t)k * (size_t)n + (size_t)i]; parts[(size_t)k * (size_t)n + (size_t)i] = 0.0; }
    if (sum != 0.0) tally[i] += sum;
}

__global__ void k_s_add2(double *p, double a, double b) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { p[0] += a; p[1] += b; }
}

// ---------------------------------------------------------------------------------------------------------------
// Owner of a slot's workspace: every array StreamWs points to, and the sizes, which describe only what is allocated.  The kernels
// get view().
struct StreamBuffers {
    long long cap = 0, room = 0, q3_cap = 0, act_room = 0, pl_room = 0, tally_n = 0;      // (as in StreamWs)
    DevBuf<SRayGeo> geo;
    DevBuf<SRayAux> aux;
    DevBuf<float4> q1_a, q1_b;
    DevBuf<SCand> q3n;
    DevBuf<uint32_t> q1_slot, q3_slot, q3_surf, hit_slot, hit_surf, gen_list, fq_ray, fq_cell, act[2], pl_slot[TRC_CLS_COUNT], pl_surf[TRC_CLS_COUNT];
    DevBuf<double> hit_t, tally_part, pl_t[TRC_CLS_COUNT];
    DevBuf<unsigned long long> hit_state, cnt;

    StreamWs view() const {
        StreamWs W;
        W.cap = cap; W.room = room; W.q3_cap = q3_cap; W.act_room = act_room; W.pl_room = pl_room; W.tally_n = tally_n;
        W.geo = geo.get(); W.aux = aux.get(); W.q1_slot = q1_slot.get(); W.q1_a = q1_a.get(); W.q1_b = q1_b.get();
        W.q3_slot = q3_slot.get(); W.q3_surf = q3_surf.get(); W.q3n = q3n.get();
        W.hit_slot = hit_slot.get(); W.hit_surf = hit_surf.get(); W.hit_t = hit_t.get();
        W.gen_list = gen_list.get(); W.fq_ray = fq_ray.get(); W.fq_cell = fq_cell.get(); W.act[0] = act[0].get(); W.act[1] = act[1].get();
        W.tally_part = tally_part.get(); W.hit_state = hit_state.get(); W.cnt = cnt.get();
        for (int c = 0; c < TRC_CLS_COUNT; ++c) { W.pl_slot[c] = pl_slot[c].get(); W.pl_surf[c] = pl_surf[c].get(); W.pl_t[c] = pl_t[c].get(); }
        return W;
    }
    // doubles the candidate queue (contents are not kept: the bounce is run again)
    int grow_q3() {
        const long long want = 2 * q3_cap;
        if (want >= (1ll << 31)) return trc_fail(TRC_ERR_CAPACITY, "candidate queue cannot grow beyond 2^31 entries (ray records link candidates by 32-bit index)");
        q3_cap = 0;
        TRC_TRY(q3_slot.alloc((size_t)want));
        TRC_TRY(q3_surf.alloc((size_t)want));
        TRC_TRY(q3n.alloc((size_t)want));
        q3_cap = want;
        return TRC_OK;
    }
};

#define STREAM_MAX_SLOTS 4
// the environment knobs of the streaming engine (StreamKnobs, trc_forms.h), read at every call
static StreamKnobs stream_knobs() {
    StreamKnobs K;
    const char *ev;
    K.search = (ev = getenv("TRC_STREAM_SEARCH")) ? atoi(ev) : 2;
    K.fresh = !((ev = getenv("TRC_STREAM_FRESH")) && !atoi(ev));
    K.bounce = !((ev = getenv("TRC_STREAM_BOUNCE")) && !atoi(ev));
    K.first = (ev = getenv("TRC_STREAM_FIRST")) && atoi(ev);
    K.coop = !((ev = getenv("TRC_STREAM_COOP")) && !atoi(ev));
    K.absorb = (ev = getenv("TRC_STREAM_ABSORB")) ? atoi(ev) : -1;
    K.static_chunks = !((ev = getenv("TRC_STREAM_STATIC")) && !atoi(ev));
    K.room_set = (ev = getenv("TRC_STREAM_ROOM")) != nullptr;
    K.room = K.room_set && atoll(ev) >= 64 ? atoll(ev) : 0;
    K.q3_entries = (ev = getenv("TRC_STREAM_Q3_ENTRIES")) && atoll(ev) > 0 ? atoll(ev) : 0;
    K.fp_cells = (ev = getenv("TRC_STREAM_FP_CELLS")) && atoi(ev) >= 32 ? atoi(ev) : 0;
    K.umask = !((ev = getenv("TRC_STREAM_UMASK")) && !atoi(ev));
    K.slots = (ev = getenv("TRC_STREAM_SLOTS")) ? atoi(ev) : 2;
    if (K.slots < 1 || K.slots > STREAM_MAX_SLOTS) K.slots = 2;
    K.clear = !((ev = getenv("TRC_STREAM_CLEAR")) && !atoi(ev));
    K.ahead = !((ev = getenv("TRC_STREAM_AHEAD")) && !atoi(ev));
    return K;
}

#define STREAM_ACT_STATIC(cap) ((cap) + ((cap) >> 2) + (1ll << 23))      /* entries of an active list that pre-assigned chunks may take */

// the queues and lists of a workspace that has none, for batches of `cap` rays
static int stream_ws_alloc_queues(StreamBuffers &W, long long cap, long long want_q3, long long want_room, const StreamKnobs &K) {
    const size_t cq = (size_t)want_room;   // (= SQ_ROOM)
    // active lists: pre-assigned chunks for at most STREAM_ACT_STATIC(cap) entries, and behind them every ray of the batch through
    // further reservations, of which every wave may leave one chunk unused -- at most as much again (TRC_STREAM_ROOM: as the
    // other lists).  Whatever the shares of the classes turn out to be, the lists cannot overflow.
    const long long act_room = K.room ? want_room
                             : 2 * STREAM_ACT_STATIC(cap) + cap + (1ll << 20);
    TRC_TRY(W.geo.alloc(cq));       // slots are handed out in chunks too
    TRC_TRY(W.aux.alloc(cq));
    TRC_TRY(W.q1_slot.alloc(cq));
    TRC_TRY(W.q1_a.alloc(cq));
    TRC_TRY(W.q1_b.alloc(cq));
    TRC_TRY(W.q3_slot.alloc((size_t)want_q3));
    TRC_TRY(W.q3_surf.alloc((size_t)want_q3));
    TRC_TRY(W.q3n.alloc((size_t)want_q3));
    TRC_TRY(W.hit_slot.alloc(cq));
    TRC_TRY(W.hit_surf.alloc(cq));
    TRC_TRY(W.hit_t.alloc(cq));
    TRC_TRY(W.gen_list.alloc(cq));
    TRC_TRY(W.fq_ray.alloc(cq));
    TRC_TRY(W.fq_cell.alloc(cq));
    TRC_TRY(W.act[0].alloc((size_t)act_room));
    TRC_TRY(W.act[1].alloc((size_t)act_room));
    TRC_TRY(W.cnt.alloc(CN_WORDS));
    TRC_TRY(W.hit_state.alloc(2 * SHADE_MAX_WAVES));        // (wave w of every shading kernel of the slot continues the chunk wave w left open)
    HIP_TRY(hipMemset(W.hit_state.get(), 0, 2 * SHADE_MAX_WAVES * sizeof(unsigned long long)));
    W.cap = cap; W.room = want_room; W.q3_cap = want_q3; W.act_room = act_room;      // (last: a workspace half made claims nothing)
    return TRC_OK;
}

static int stream_ws_alloc(StreamBuffers &W, long long cap, int n_unbounded, long long tally_n, const StreamKnobs &K) {
    // candidate pairs per bounce: 4 per ray to start with (NSTTF needs 0.25); a bounce that overflows is run again with
    // twice the room.  TRC_STREAM_Q3_ENTRIES (tests) sets the initial capacity.
    long long want_q3 = (4 + (long long)n_unbounded) * cap + (long long)SQ_CHUNK_MAX * 16384;
    if (K.q3_entries) want_q3 = K.q3_entries;
    long long want_room = cap + (long long)SQ_CHUNK_MAX * 16384;   // room for the invalid tails of every wave's last chunk
    if (K.room) want_room = K.room;      // tests: lists that overflow
    if (!(W.cap >= cap && W.q3_cap >= want_q3 && (K.room ? W.room == want_room : W.room >= want_room))) {
        W = StreamBuffers();      // the class lists and the private tallies go with the queues
        TRC_TRY(stream_ws_alloc_queues(W, cap, want_q3, want_room, K));
    }
    if (W.tally_n != tally_n || !W.tally_part) {      // flux maps may have been added since the last call
        W.tally_n = 0;
        TRC_TRY(W.tally_part.alloc((size_t)TALLY_PARTS * (size_t)tally_n));
        HIP_TRY(hipMemset(W.tally_part.get(), 0, (size_t)TALLY_PARTS * (size_t)tally_n * sizeof(double)));
        W.tally_n = tally_n;
    }
    return TRC_OK;
}

// One batch in flight: its workspace, its stream and where it is in its bounces.  Two of them alternate, so that the
// arithmetic-bound kernels of one batch (generation, walk) share the device with the access-bound ones of the other
// (exact tests, tie pass, shading).
struct StreamSlot {
    StreamBuffers W;
    DevBuf<double> spec;          // spectra of the rays under way (CarryIn.slot_spec), spec_len doubles; spec_on: this call brings spectra
    long long spec_len = 0;
    bool spec_on = false;
    // a call whose optics split rays (k_s_shade_x<.., SPLIT>): the Philox stream of the ray in every slot (CarryIn.slot_rid, rid_len
    // entries), the slots handed out by the bounces done, and the slots a wave of the shading kernel reserves per atomic
    DevBuf<unsigned long long> rid;
    long long rid_len = 0;
    unsigned long long slots_used = 0;
    unsigned chunk_slot_sh = SQ_CHUNK;
    StreamHandle stream;          // slot 0 borrows the context's stream, which is not this slot's to destroy; the others own theirs
    EventHandle done;
    PinnedWords h_cnt;            // pinned: CN_WORDS counters read back, then CN_WORDS counters to upload
    StreamParams SP;              // (assigned by start_batch)
    long long base = 0, nb = 0, n_in = 0;
    unsigned long long n_act = 0;
    int b = 0, cur = 0, attempt = 0;
    unsigned gb_wide = 0, gb_gen = 0, gb_walk = 0, gb_cull = 0, gb_fresh = 0, gb_bounce = 0;    // grids of the bounce being run
    unsigned gb_sh[TRC_CLS_COUNT] = {};            // ... of the shading kernels of the classes present
    unsigned chunk_act_sh[TRC_CLS_COUNT] = {};     // entries of the active list pre-assigned to every wave of each
    long long act_base_sh[TRC_CLS_COUNT] = {};     // ... and where its chunks start
    unsigned gb_part = 0;                          // grid of k_s_partition (0: one shading class, the hit list is walked as it is)
    unsigned long long part_start[TRC_CLS_COUNT] = {};   // entries of each class list that are pre-assigned to the waves of k_s_partition
    unsigned cull_chunk = 0;      // entries of the footprint list pre-assigned to every wave of k_s_cull
    unsigned cull_gen_chunk = 0;  // ... and of the general-path list (0: collected per workgroup, see CullParams)
    bool fresh_one = false;       // this batch's listed rays go to k_s_fresh although the source has the two-phase form
    bool umask = false;           // this batch's k_s_cull reads the mask over the uniforms, and k_s_fresh2 takes its list
    bool fresh = false, general = false, fused = false, first = false;     // first: k_s_bounce<.., FRESH> takes the fresh rays outside the footprint map
    unsigned gb_first = 0;  // this bounce: k_s_fresh generates the rays / the general path (gen, walk, exact) runs / k_s_bounce searches
    bool busy = false;
};

struct StreamEngine {
    StreamSlot slot[STREAM_MAX_SLOTS];
    bool ready = false;        // the slots have their streams, events and pinned blocks
    // footprint map of the last source traced on this scene (trc_footprint.h): rebuilt when the source or the poses change
    std::unique_ptr<trc_fp_host> fp;
    unsigned char fp_key[sizeof(int32_t) + (3 + 9 + 9 + 8) * sizeof(double)] = {};
    uint64_t fp_geom_version = 0;
    bool fp_valid = false;
    double fp_hit_rate = 0.0;  // hits per fresh ray measured on the batches traced with this map (0: not yet), + margin: sizes the chunks
    // k_s_bounce's two lists: hits per ray entering bounce b on surfaces that end the ray / on the others, measured on the batches
    // before (+ margin; < 0: not yet -- every ray may hit).  A list sized for every ray but filled by 3 % of them costs k_s_shade
    // 0.1 ms of walking over invalid entries.
#define STREAM_RATE_BOUNCES 8
    double rate_term[STREAM_RATE_BOUNCES], rate_other[STREAM_RATE_BOUNCES];
    double rate_cls[STREAM_RATE_BOUNCES][TRC_CLS_COUNT];   // hits per ray entering bounce b that each shading class took (< 0: not yet)
    // rays per ray entering bounce b that its shading left on the active list, measured on the batches whose shading finished the
    // others' next segment itself (StreamParams.ahead; < 0: not yet): sizes the chunks of that list, and with them the next bounce
    double rate_left[STREAM_RATE_BOUNCES];
    uint64_t rate_geom_version = 0;      // the pose the rates were measured on
    DevBuf<uint32_t> d_fp_mask, d_fp_coff, d_fp_umask;     // (d_fp_umask: empty where the source's kernels do not use the mask over the uniforms)
    DevBuf<uint32_t> d_fp_clist;

    void forget_rates() {      // not measured yet
        for (int b = 0; b < STREAM_RATE_BOUNCES; ++b) { rate_term[b] = rate_other[b] = rate_left[b] = -1.0; for (int c = 0; c < TRC_CLS_COUNT; ++c) rate_cls[b][c] = -1.0; }
    }
};

// the part of a source descriptor the footprint map depends on (the Buie table enters through p[] / the CSR only via cdf_end,
// which is compared below as well)
static void stream_fp_key(const trc_source_desc &src, unsigned char *key) {
    memcpy(key, &src.kind, sizeof(int32_t)); key += sizeof(int32_t);
    memcpy(key, src.center, 3 * sizeof(double)); key += 3 * sizeof(double);
    memcpy(key, src.rot_pos, 9 * sizeof(double)); key += 9 * sizeof(double);
    memcpy(key, src.rot_dir, 9 * sizeof(double)); key += 9 * sizeof(double);
    memcpy(key, src.p, 8 * sizeof(double));
}

// Makes (or finds) the footprint map of `src` over the scene.  *use = false when the map does not apply to this source / scene
// (the general path then generates every ray).  TRC_STREAM_FRESH=0 switches the map off (tests compare the two paths).
static int stream_fp_prepare(trc_scene *sc, StreamEngine &E, const trc_source_desc *src, const StreamKnobs &K, FpDev *out, bool *use) {
    *use = false;
    if (!K.fresh || !src) return TRC_OK;
    unsigned char key[sizeof(E.fp_key)];
    stream_fp_key(*src, key);
    const bool buie = src->kind == TRC_SRC_BUIE_DISK || src->kind == TRC_SRC_BUIE_RECT;
    const double cdf_end = buie ? src->buie[2 * (TRC_BUIE_NELEM + 1) + TRC_BUIE_NELEM] : 0.0;
    if (!E.fp) { E.fp.reset(new (std::nothrow) trc_fp_host()); if (!E.fp) return trc_fail(TRC_ERR_NOMEM, "out of host memory"); E.fp_valid = false; }
    if (!(E.fp_valid && E.fp_geom_version == sc->search.geom_version() && memcmp(key, E.fp_key, sizeof(key)) == 0 && (!buie || E.fp->P.cdf_end == cdf_end))) {
        int M = sc->n_surf > 4096 ? 1024 : 512;       // (a mesh of small faces: finer cells, fewer faces listed per cell; the mask still fits k_s_cull's LDS)
        const bool forced = K.fp_cells > 0;
        const bool um = buie;      // the mask over the uniforms: for the sources whose listed rays go to k_s_fresh2 (trc_stream_form_fresh)
        if (forced) M = K.fp_cells;
        if (M > 1024) M = 1024;
        if (sc->n_surf > 4096 && !forced) {
            // A large mesh that fills the source's view: nearly every ray starts over a face, the map culls nothing, and building
            // it at full resolution takes seconds (1e5 faces: 2.5 s).  A coarse map first (1/16 of the work): covered more than
            // 80 % -> no map for this scene and source, every fresh ray is searched on the grid (k_s_bounce<.., FRESH>).
            trc_fp_build(sc->surfaces.data(), sc->n_surf, sc->search.host(), *src, *E.fp, 256, false);
            const bool disc = src->kind == TRC_SRC_BUIE_DISK || src->kind == TRC_SRC_PILLBOX_DISK || src->kind == TRC_SRC_SUNSHAPE_DISK;      // (the mask is a square around the disc)
            if (E.fp->ok && E.fp->coverage * (disc ? 4.0 / TRC_PI : 1.0) > 0.8) E.fp->ok = false;
            else trc_fp_build(sc->surfaces.data(), sc->n_surf, sc->search.host(), *src, *E.fp, M, um);
        } else
        trc_fp_build(sc->surfaces.data(), sc->n_surf, sc->search.host(), *src, *E.fp, M, um);
        memcpy(E.fp_key, key, sizeof(key));
        E.fp_geom_version = sc->search.geom_version();
        E.fp_valid = true;
        E.fp_hit_rate = 0.0;
        E.d_fp_mask.reset(); E.d_fp_coff.reset(); E.d_fp_clist.reset(); E.d_fp_umask.reset();
        if (E.fp->ok && !E.fp->umask.empty()) TRC_TRY(dev_upload(E.d_fp_umask, E.fp->umask.data(), E.fp->umask.size()));
        if (E.fp->ok) {
            TRC_TRY(dev_upload(E.d_fp_mask, E.fp->mask.data(), E.fp->mask.size()));
            TRC_TRY(dev_upload(E.d_fp_coff, E.fp->coff.data(), E.fp->coff.size()));
            TRC_TRY(dev_upload(E.d_fp_clist, E.fp->clist.data(), E.fp->clist.size()));
        }
    }
    if (!E.fp->ok) return TRC_OK;
    out->P = E.fp->P;
    out->mask = E.d_fp_mask.get(); out->coff = E.d_fp_coff.get(); out->clist = E.d_fp_clist.get();
    out->n_list = (long long)E.fp->clist.size();
    *use = true;
    return TRC_OK;
}

// streams, events and pinned counter blocks of the slots, made once
static int stream_engine_init(StreamEngine *E, trc_ctx *ctx) {
    if (E->ready) return TRC_OK;
    E->forget_rates();
    for (int k = 0; k < STREAM_MAX_SLOTS; ++k) {
        StreamSlot &T = E->slot[k];
        hipStream_t st;
        hipEvent_t ev;
        unsigned long long *h;
        if (k == 0) T.stream.borrow(ctx->stream);
        else { HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); T.stream.own(st); }
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        T.done.own(ev);
        HIP_TRY(hipHostMalloc((void **)&h, 2 * CN_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
        T.h_cnt.own(h);
    }
    E->ready = true;
    return TRC_OK;
}

// A kernel id (trc_forms.h) -> the instance the library holds for it, null: none.  One place per family, which reads nothing but the
// id; the ids a place answers with a pointer are those of trc_kernel_id_valid, and the kernels compiled are exactly these.
// ... the families whose first argument is the source kind: k_s_cull, k_s_ucull, k_s_fresh, k_s_fresh2
template <int KIND, bool FLAT, bool LDS>
static const void *fresh_kernel_of(int family) {
    if (family == TRC_K_FRESH) return (const void *)k_s_fresh<KIND, FLAT, LDS>;
    if constexpr (KIND == TRC_SRC_BUIE_DISK || KIND == TRC_SRC_BUIE_RECT) if (family == TRC_K_FRESH2) return (const void *)k_s_fresh2<KIND, FLAT, LDS>;
    return nullptr;
}
template <int KIND>
static const void *source_kernel_of(const trc_kernel_id &id) {
    if (id.family == TRC_K_CULL) return (const void *)k_s_cull<KIND>;
    if constexpr (KIND == TRC_SRC_BUIE_DISK || KIND == TRC_SRC_BUIE_RECT) if (id.family == TRC_K_UCULL) return (const void *)k_s_ucull<KIND>;
    const bool flat = id.a[1] != 0, lds = id.a[2] != 0;
    return flat ? (lds ? fresh_kernel_of<KIND, true, true>(id.family) : fresh_kernel_of<KIND, true, false>(id.family))
                : (lds ? fresh_kernel_of<KIND, false, true>(id.family) : fresh_kernel_of<KIND, false, false>(id.family));
}
static const void *source_kernel_fn(const trc_kernel_id &id) {
    switch (id.a[0]) {
    case TRC_SRC_PILLBOX_DISK: return source_kernel_of<TRC_SRC_PILLBOX_DISK>(id);
    case TRC_SRC_PILLBOX_RECT: return source_kernel_of<TRC_SRC_PILLBOX_RECT>(id);
    case TRC_SRC_BUIE_DISK: return source_kernel_of<TRC_SRC_BUIE_DISK>(id);
    case TRC_SRC_BUIE_RECT: return source_kernel_of<TRC_SRC_BUIE_RECT>(id);
    case TRC_SRC_SUNSHAPE_DISK: return source_kernel_of<TRC_SRC_SUNSHAPE_DISK>(id);
    case TRC_SRC_SUNSHAPE_RECT: return source_kernel_of<TRC_SRC_SUNSHAPE_RECT>(id);
    default: return nullptr;
    }
}
// ... k_s_gen, k_s_gen_src
static const void *gen_kernel_fn(const trc_kernel_id &id) {
    const int kind = id.family == TRC_K_GEN ? id.a[1] : id.a[0];
    if (id.family == TRC_K_GEN_EMIT) return (const void *)k_s_gen_emit;
    if (id.family == TRC_K_GEN_LAMP)
        return kind == TRC_SRC_ARC_VOLUME ? (const void *)k_s_gen_lamp<TRC_SRC_ARC_VOLUME> : kind == TRC_SRC_EMIT_SPHERE ? (const void *)k_s_gen_lamp<TRC_SRC_EMIT_SPHERE>
             : kind == TRC_SRC_EMIT_CYLINDER ? (const void *)k_s_gen_lamp<TRC_SRC_EMIT_CYLINDER> : nullptr;
    if (id.family == TRC_K_GEN_SRC)
        return kind == TRC_SRC_BUIE_DISK ? (const void *)k_s_gen_src<TRC_SRC_BUIE_DISK> : kind == TRC_SRC_PILLBOX_DISK ? (const void *)k_s_gen_src<TRC_SRC_PILLBOX_DISK>
             : kind == TRC_SRC_PILLBOX_RECT ? (const void *)k_s_gen_src<TRC_SRC_PILLBOX_RECT> : nullptr;
    if (!id.a[0]) return kind == -1 ? (const void *)k_s_gen<false> : nullptr;
    return kind == -1 ? (const void *)k_s_gen<true> : kind == TRC_SRC_BUIE_RECT ? (const void *)k_s_gen<true, TRC_SRC_BUIE_RECT>
         : kind == TRC_SRC_SUNSHAPE_DISK ? (const void *)k_s_gen<true, TRC_SRC_SUNSHAPE_DISK>
         : kind == TRC_SRC_SUNSHAPE_RECT ? (const void *)k_s_gen<true, TRC_SRC_SUNSHAPE_RECT> : nullptr;
}
// ... k_s_bounce, k_s_bounce_coop
template <bool FRESH, bool FLAT, bool SUN>
static const void *bounce_kernel_of(const trc_kernel_id &id) {
    if (id.family == TRC_K_BOUNCE_COOP) return (const void *)k_s_bounce_coop<FRESH, FLAT, SUN>;
    if constexpr (FRESH && FLAT) return nullptr;        // (k_s_bounce takes fresh rays in its instance for any geometry)
    else {
        const bool lds = id.a[1] != 0;
        switch (id.a[0]) {
        case 0: return lds ? (const void *)k_s_bounce<0, true, FRESH, FLAT, SUN> : (const void *)k_s_bounce<0, false, FRESH, FLAT, SUN>;
        case 1: return lds ? (const void *)k_s_bounce<1, true, FRESH, FLAT, SUN> : (const void *)k_s_bounce<1, false, FRESH, FLAT, SUN>;
        case 2: return lds ? nullptr : (const void *)k_s_bounce<2, false, FRESH, FLAT, SUN>;
        case 3: return lds ? nullptr : (const void *)k_s_bounce<3, false, FRESH, FLAT, SUN>;
        default: return nullptr;
        }
    }
}
static const void *bounce_kernel_fn(const trc_kernel_id &id) {
    const int *a = id.family == TRC_K_BOUNCE ? id.a + 2 : id.a;       // FRESH, FLAT, SUN
    const bool fresh = a[0] != 0, flat = a[1] != 0, sun = a[2] != 0;
    if (!fresh) return sun ? nullptr : flat ? bounce_kernel_of<false, true, false>(id) : bounce_kernel_of<false, false, false>(id);
    if (flat) return sun ? bounce_kernel_of<true, true, true>(id) : bounce_kernel_of<true, true, false>(id);
    return sun ? bounce_kernel_of<true, false, true>(id) : bounce_kernel_of<true, false, false>(id);
}
// ... k_s_shade
template <bool LDS, bool SPEC>
static const void *shade_kernel_of(bool simple, bool chart) {
    if (chart) return simple ? nullptr : (const void *)k_s_shade<false, 2, LDS, SPEC, true>;
    return simple ? (const void *)k_s_shade<true, 2, LDS, SPEC> : (const void *)k_s_shade<false, 2, LDS, SPEC>;
}
static const void *shade_kernel_fn(const trc_kernel_id &id) {
    const bool simple = id.a[0] != 0, lds = id.a[2] != 0, spec = id.a[3] != 0, chart = id.a[4] != 0;
    if (id.a[1] != 2) return nullptr;
    return lds ? (spec ? shade_kernel_of<true, true>(simple, chart) : shade_kernel_of<true, false>(simple, chart))
               : (spec ? shade_kernel_of<false, true>(simple, chart) : shade_kernel_of<false, false>(simple, chart));
}
// ... and every family of the streaming engine (the lean and carry kernels: trc_shade.hip)
static const void *stream_kernel_fn(const trc_kernel_id &id) {
    switch (id.family) {
    case TRC_K_CULL: case TRC_K_UCULL: case TRC_K_FRESH: case TRC_K_FRESH2: return source_kernel_fn(id);
    case TRC_K_GEN: case TRC_K_GEN_SRC: case TRC_K_GEN_LAMP: case TRC_K_GEN_EMIT: return gen_kernel_fn(id);
    case TRC_K_BOUNCE: case TRC_K_BOUNCE_COOP: return bounce_kernel_fn(id);
    case TRC_K_WALK: return id.a[0] != SW_THREADS ? nullptr : id.a[1] ? (const void *)k_s_walk<SW_THREADS, true> : (const void *)k_s_walk<SW_THREADS, false>;
    case TRC_K_EXACT: return (const void *)k_s_exact;
    case TRC_K_ABSORB: return (const void *)k_s_absorb;
    case TRC_K_SHADE: return shade_kernel_fn(id);
    case TRC_K_SHADE_C: return trc_shade_lean_kernel(id.a[0], id.a[1] != 0, id.a[2] != 0, id.a[3] != 0, id.a[4] != 0);
    case TRC_K_SHADE_X: return trc_shade_carry_kernel(id.a[0] != 0, id.a[1] != 0, id.a[2] != 0, id.a[3] != 0);
    case TRC_K_SHADE_P: return trc_shade_poly_kernel(id.a[0] != 0, id.a[1] != 0, id.a[2] != 0);
    default: return nullptr;
    }
}

// one kernel instance of a stage as the batches launch it: the function of its id, threads per workgroup, dynamic LDS, and the grid
// cap (the workgroups resident at once)
struct StreamKernel { const void *fn; int threads; size_t lds; unsigned max_blocks; };
// ... of a shading kernel: the class it serves (-1: the only shading kernel, every kind) and the tables it stages
struct StreamShadeK { int cls; const void *fn; unsigned threads, wpb, max_blocks; size_t lds; int lds_tables, lds_fm_bins; };

// The kernels a call runs: the decisions (D, trc_forms.h) and, stage by stage, the instance they name made ready to launch
struct StreamForms {
    trc_stream_forms D;
    StreamKernel gen0, gen, walk, exact;     // the general path (grids: g_gen, walk.max_blocks, g_wide)
    unsigned g_gen, g_wide;      // (g_wide: k_s_partition too)
    StreamShadeK shk[TRC_CLS_COUNT];
    StreamKernel cull, fresh, fresh_one, cull_u;
    CullParams cull_up;          // what k_s_ucull takes that k_s_cull does not: the mask, its words and dimensions, the generic compare
    StreamKernel bounce, first, absorb;
};

// A stage made ready: the function of its id (a missing one is an error), its grid cap at `lds_cap` bytes (cap) and the leave to take
// its dynamic LDS.  A stage the call does not have (TRC_K_NONE) stays empty.
static int stream_stage(StreamKernel &k, const trc_stage &s, int n_cu, bool cap, size_t lds_cap) {
    k = {nullptr, s.threads, s.lds, 0u};
    if (s.id.family == TRC_K_NONE) return TRC_OK;
    k.fn = stream_kernel_fn(s.id);
    if (!k.fn) {
        char name[96];
        trc_kernel_name(s.id, name, sizeof(name));
        return trc_fail(TRC_ERR_UNSUPPORTED, "the library holds no kernel %s", name);
    }
    if (cap) TRC_TRY(kernel_grid_cap(k.fn, k.threads, lds_cap, 2048 / k.threads, n_cu, &k.max_blocks));
    return (cap && lds_cap == k.lds) ? TRC_OK : kernel_allow_lds(k.fn, k.lds);
}

// Chooses the kernel of every stage for this call and sets up SP0, the parameters every batch starts from: the facts are gathered,
// trc_stream_decide (trc_forms.h) decides, each id chosen becomes a function, and each function gets its grid cap and its LDS
static int stream_choose_forms(StreamForms &F, StreamParams &SP0, trc_scene *sc, StreamEngine &E, const StreamPlan &plan, trc_facts &f,
                               const trc_source_desc *src_desc) {
    const int n_cu = sc->ctx->n_cu;
    memset(&F, 0, sizeof(F));
    // 1. the facts the call did not have yet: the pass over the surfaces, and the footprint map of the source
    f.scene = scene_facts(sc, true);
    f.fp = {};
    TRC_TRY(stream_fp_prepare(sc, E, src_desc, f.knobs, &SP0.fp, &f.fp.use));
    if (f.fp.use) {
        const trc_fp_host &H = *E.fp;
        f.fp = {true, SP0.fp.n_list, H.P.M, H.P.Mc, H.P.has_generic != 0, H.P.cdf_end, H.coverage, H.ucoverage, E.d_fp_umask.get() ? (int)H.umask.size() : 0, H.Mu, H.Mv};
    }
    // 2. the decisions
    trc_stream_forms &D = F.D;
    if (!trc_stream_decide(f, plan, &D)) return trc_fail(TRC_ERR_UNSUPPORTED, "no shading kernel for device material tables beside a chart flux map");
    SP0.search = D.search; SP0.lds_recs = D.lds_recs; SP0.P.lds_tally = D.lds_tally; SP0.lds_tables = D.lds_tables; SP0.lds_extra = D.lds_extra;
    SP0.lds_fm_bins = D.lds_fm_bins; SP0.bg_occ_words = D.bg_occ_words; SP0.shade_term_cls = D.shade_term_cls; SP0.split_terminal = D.split_terminal;
    SP0.carry.poly_cells = D.poly_cells;
    SP0.clear_tab = f.knobs.clear ? sc->search.clear_cones() : nullptr;
    SP0.ahead = (D.ahead && SP0.clear_tab) ? 1 : 0;
    SP0.hit_epoch = sc->hits.epoch;
    SP0.chunk_hitbuf = sc->hits.chunk_size();
    // 3. and 4. the instances, their grid caps and their LDS
    TRC_TRY(stream_stage(F.gen0, D.gen0, n_cu, false, 0));
    TRC_TRY(stream_stage(F.gen, D.gen, n_cu, false, 0));
    TRC_TRY(stream_stage(F.walk, D.walk, n_cu, true, D.walk.lds));
    TRC_TRY(stream_stage(F.exact, D.exact, n_cu, false, 0));
    F.g_wide = (unsigned)(n_cu * 8);     // 256-thread blocks: 4 waves each, <= 16384 waves in all
    F.g_gen = (unsigned)(n_cu * 8);
    for (int q = 0; q < D.n_shk; ++q) {
        const trc_shade_stage &s = D.shk[q];
        StreamKernel k;
        // k_s_shade: 2 waves per SIMD, four workgroups of 256 per CU in two rounds; the others by their occupancy, within the waves
        // that may keep a chunk of the hit buffer open
        const bool cap = s.id.family != TRC_K_SHADE;
        TRC_TRY(stream_stage(k, {s.id, s.threads, s.lds}, n_cu, cap, s.lds));
        StreamShadeK &K = F.shk[q];
        K = {s.cls, k.fn, (unsigned)s.threads, (unsigned)s.threads / 64, cap ? k.max_blocks : (unsigned)(n_cu * 4), s.lds, s.lds_tables, s.lds_fm_bins};
        if (cap && (unsigned long long)K.max_blocks * K.wpb > SHADE_MAX_WAVES) K.max_blocks = SHADE_MAX_WAVES / K.wpb;
    }
    TRC_TRY(stream_stage(F.cull, D.cull, n_cu, true, D.cull.lds));
    TRC_TRY(stream_stage(F.fresh, D.fresh, n_cu, true, D.fresh.lds));
    if (trc_kid_equal(D.fresh_one.id, D.fresh.id)) F.fresh_one = {F.fresh.fn, F.fresh.threads, F.fresh.lds, 0u};
    else TRC_TRY(stream_stage(F.fresh_one, D.fresh_one, n_cu, false, 0));
    TRC_TRY(stream_stage(F.cull_u, D.cull_u, n_cu, true, D.cull_u.lds));
    if (F.cull_u.fn) {
        CullParams &U = F.cull_up;
        U.mask = E.d_fp_umask.get(); U.mask_words = (int)E.fp->umask.size();
        U.lu = D.cull_lu; U.lv = D.cull_lv;
        bool on;
        U.gen_thr = trc_fp_generic_threshold(SP0.fp.P, &on);
        U.gen_on = on ? 1 : 0;
    }
    // (k_s_bounce keeps the grid cap of its LDS without k_s_absorb's tables)
    TRC_TRY(stream_stage(F.bounce, D.bounce, n_cu, true, D.bounce.lds - D.lds_inline));
    TRC_TRY(stream_stage(F.first, D.first, n_cu, true, D.first.lds));
    // k_s_absorb: one workgroup of 16 waves per CU (4096 waves with open chunks of the hit buffer at most)
    TRC_TRY(stream_stage(F.absorb, D.absorb, n_cu, false, 0));
    if (F.absorb.fn) F.absorb.max_blocks = (unsigned)n_cu;
    return TRC_OK;
}

// workspaces of the slots for batches of `cap` rays: queues, spectra of the rays under way, the class lists of k_s_partition
static int stream_slots_alloc(StreamEngine &E, int n_slots, long long cap, const trc_scene *sc, const CarryIn &carry_in, const StreamForms &F, const StreamKnobs &K,
                              bool split_rays, bool poly_src) {
    for (int k = 0; k < n_slots; ++k) {
        StreamSlot &Tk = E.slot[k];
        TRC_TRY(stream_ws_alloc(Tk.W, cap, (int)sc->search.host().unbounded.size(), (long long)sc->tally.size(), K));
        // (a source that carries its spectrum brings no columns, but its rays' spectra live in the slot table all the same)
        const long long want = ((carry_in.spec || poly_src) && carry_in.n_spec > 0) ? (long long)carry_in.n_spec * Tk.W.room : 0;
        if (Tk.spec_len < want) {
            Tk.spec_len = 0;
            TRC_TRY(Tk.spec.alloc((size_t)want));
            Tk.spec_len = want;
        }
        Tk.spec_on = want > 0;
        if (split_rays && Tk.rid_len < Tk.W.room) {
            Tk.rid_len = 0;
            TRC_TRY(Tk.rid.alloc((size_t)Tk.W.room));
            Tk.rid_len = Tk.W.room;
        }
        StreamBuffers &Wk = Tk.W;
        if (!F.D.multi) continue;
        Wk.pl_room = 2 * Wk.room;
        for (int q = 0; q < F.D.n_shk; ++q) {
            const int c = F.shk[q].cls;
            if (Wk.pl_t[c]) continue;      // (the last of the three made: a list half made is made again)
            TRC_TRY(Wk.pl_slot[c].alloc((size_t)Wk.pl_room));
            TRC_TRY(Wk.pl_surf[c].alloc((size_t)Wk.pl_room));
            TRC_TRY(Wk.pl_t[c].alloc((size_t)Wk.pl_room));
        }
    }
    return TRC_OK;
}

// One call: its forms, the parameters every batch starts from, the batch size, and what the batches add up to
struct StreamCall {
    const StreamForms &F;
    const StreamKnobs &K;
    StreamEngine &E;
    StreamParams SP0;
    long long cap;
    double seg, hits;
    double cls_hits[TRC_CLS_COUNT];      // hits shaded by the kernel of each class (first STREAM_RATE_BOUNCES bounces)
    int launches, max_bounces;
    bool split_rays;                     // the scene's optics can send two rays on from a hit (k_s_shade_x<.., SPLIT>)
};

// a grid of g workgroups, at least one and at most max_blocks
static unsigned clamp_grid(long long g, unsigned max_blocks) { return (unsigned)(g < 1 ? 1 : (g > (long long)max_blocks ? (long long)max_blocks : g)); }

// grids and reservation sizes of a slot's next bounce
static void plan_bounce(const StreamCall &C, StreamSlot &T) {
    const StreamForms &F = C.F;
    const StreamEngine &E = C.E;
    // Grids follow the work of the bounce (every kernel strides over its queue, so a small grid is only slower, never
    // wrong), with at least SW_ITEMS items per thread: later bounces and small calls do not pay for 2048 workgroups
    // staging their tables.
    long long work = T.b == 0 ? T.nb : (long long)T.n_act;
    auto grid_for = [&](unsigned max_blocks, int threads) { return clamp_grid((work + threads - 1) / threads, max_blocks); };
    // one pre-assigned chunk per appending wave, for `expected` entries over `waves` waves (+ margin): a multiple of 64, at
    // least SQ_CHUNK, and never more than the lists have room for
    auto chunk_for = [&](double expected, unsigned long long waves, unsigned floor = SQ_CHUNK) {
        double c = 1.1 * expected / (double)(waves ? waves : 1ull) + (floor < SQ_CHUNK ? 48.0 : 128.0);
        const double most = 0.9 * (double)T.W.room / (double)(waves ? waves : 1ull);
        if (c > most) c = most;
        unsigned u = ((unsigned)c + 63u) & ~63u;
        return u < floor ? floor : u;
    };
    const int sf_threads = F.fresh.threads, sb_threads = F.bounce.threads, first_threads = F.first.threads;
    T.fresh = F.D.use_fp && T.b == 0;
    T.fused = F.D.use_fused && T.b > 0;
    T.first = F.D.use_first && T.b == 0 && (!T.fresh || F.D.general_share > 0.0);
    T.general = !T.fused && !T.first && (!T.fresh || F.D.general_share > 0.0);
    T.gb_bounce = T.fused ? grid_for(F.bounce.max_blocks, sb_threads) : 0u;
    T.gb_cull = T.fresh ? grid_for(F.cull.max_blocks, SC_THREADS * 8) : 0u;
    T.SP.chunk_hit = T.SP.chunk_slot = T.SP.chunk_act = T.SP.chunk_first = T.SP.chunk_thit = SQ_CHUNK;
    double act_expected = -1.0;          // rays expected to go on from this bounce's shading (< 0: unknown, the waves reserve as they go)
    long long shade_entries = work;      // entries of the hit list the shading kernels walk (used or not)
    T.gb_first = 0u;
    T.cull_chunk = SQ_CHUNK;
    T.cull_gen_chunk = 0;
    T.umask = false;
    if (T.fresh) {        // one lane per listed ray, a few rays per lane
        // the two-phase form pays where most listed rays miss (a field of mirrors: two of three); where most of them hit (a dish
        // under its own source: the first phase rejects nothing) the batches after the first go back to k_s_fresh, which is
        // handed its cells by k_s_cull on the Cartesian mask
        const bool mostly_hits = E.fp_hit_rate > 0.0 && E.fp_hit_rate > 0.6 * 1.15 * F.D.listed_share;
        T.umask = F.cull_u.fn != nullptr && !mostly_hits;
        T.fresh_one = mostly_hits;
        if (T.umask) T.gb_cull = grid_for(F.cull_u.max_blocks, SC_THREADS * 8);
        // (the mask over the uniforms lists somewhat more rays than the Cartesian one: its lists and grids are sized by its own share)
        const double listed = (T.umask ? F.D.ulisted_share : F.D.listed_share) * (double)T.nb;
        T.gb_fresh = clamp_grid(((long long)(1.2 * listed) + 4096 + sf_threads * 2 - 1) / (sf_threads * 2), F.fresh.max_blocks);
        T.cull_chunk = chunk_for(1.1 * listed, (unsigned long long)T.gb_cull * (SC_THREADS / 64));
        // general-path rays: rare -> per workgroup through LDS; a source with a strong aureole (CSR 0.3: a third of the rays) ->
        // chunks per wave like the other lists
        if (F.D.general_share * (double)T.nb / (double)T.gb_cull > 0.25 * SC_GEN_CAP)
            T.cull_gen_chunk = chunk_for(1.1 * F.D.general_share * (double)T.nb, (unsigned long long)T.gb_cull * (SC_THREADS / 64));
        // hits of the fresh rays: measured on the batches before (E.fp_hit_rate), every listed ray to start with
        const double hits = (E.fp_hit_rate > 0.0 ? E.fp_hit_rate : (T.umask ? F.D.ulisted_share : F.D.listed_share)) * (double)T.nb;
        T.SP.chunk_hit = T.SP.chunk_slot = chunk_for(hits, (unsigned long long)T.gb_fresh * (unsigned long long)(sf_threads / 64));
        act_expected = hits + 2.0 * F.D.general_share * (double)T.nb;
    } else {
        T.gb_fresh = 0u;
        if (T.fused) {    // at most the rays that entered the bounce hit, at most those go on
            const unsigned long long bw = (unsigned long long)T.gb_bounce * (unsigned long long)(sb_threads / 64);
            const bool known = T.b < STREAM_RATE_BOUNCES && E.rate_term[T.b] >= 0.0;
            // (the few hits that are left to k_s_shade behind k_s_absorb: short chunks, its list is walked entry by entry)
            T.SP.chunk_hit = chunk_for((known ? E.rate_other[T.b] : 1.0) * (double)T.n_in, bw, (known && C.SP0.split_terminal) ? 64u : (unsigned)SQ_CHUNK);
            T.SP.chunk_thit = chunk_for((known ? E.rate_term[T.b] : 1.0) * (double)T.n_in, bw);
            // the shading kernels only see the hits that k_s_absorb does not take: grids for the entries of their list, used or not
            // (every workgroup stages 50 KB of tables and flushes its private sums, hits or not)
            if (known && (long long)bw * (long long)T.SP.chunk_hit < shade_entries) shade_entries = (long long)bw * (long long)T.SP.chunk_hit;
            act_expected = (known && C.SP0.split_terminal ? E.rate_other[T.b] : 1.0) * (double)T.n_in;
        }
    }
    // behind k_s_cull the general path only sees the rays left to it (the Buie aureole)
    if (T.fresh) work = (long long)(1.5 * F.D.general_share * (double)T.nb) + 4096;
    if (T.first) {
        T.gb_first = grid_for(F.first.max_blocks, first_threads);
        T.SP.chunk_first = chunk_for((double)work, (unsigned long long)T.gb_first * (first_threads / 64));      // at most every ray hits
        if (!T.fresh) act_expected = (double)work;
    }
    // the shading kernels of the classes present: grids, and their parts of the active list
    {
        const double rays_in0 = T.b == 0 ? (double)T.nb : (double)T.n_in;
        long long entries_of[TRC_CLS_COUNT] = {shade_entries, shade_entries, shade_entries};
        T.gb_part = 0u;
        for (int c = 0; c < TRC_CLS_COUNT; ++c) { T.part_start[c] = 0ull; T.SP.part_chunk[c] = SQ_CHUNK_MAX; T.SP.part_static[c] = 0; }
        if (F.D.multi) {
            T.gb_part = clamp_grid((shade_entries + 256ll * SW_ITEMS - 1) / (256ll * SW_ITEMS), F.g_wide);
            const unsigned long long pw = (unsigned long long)T.gb_part * 4ull;
            for (int k = 0; k < F.D.n_shk; ++k) {
                const int c = F.shk[k].cls;
                if (!(C.K.static_chunks && T.b < STREAM_RATE_BOUNCES && E.rate_cls[T.b][c] >= 0.0)) continue;      // share not known yet: the waves reserve as they go
                double cc = 1.1 * E.rate_cls[T.b][c] * rays_in0 / (double)pw + 128.0;
                const double most = (double)T.W.room / (double)pw - 64.0;
                if (cc > most) cc = most;
                unsigned chunk = ((unsigned)cc + 63u) & ~63u;
                if (chunk < SQ_CHUNK) chunk = SQ_CHUNK;
                T.SP.part_chunk[c] = chunk;
                T.SP.part_static[c] = 1;
                T.part_start[c] = pw * (unsigned long long)chunk;
                if ((long long)T.part_start[c] < entries_of[c]) entries_of[c] = (long long)T.part_start[c];
            }
        }
        unsigned long long total_waves = 0;
        for (int k = 0; k < F.D.n_shk; ++k) {
            const long long per = (long long)F.shk[k].threads * SW_ITEMS;
            const long long shade_entries_k = F.D.multi ? entries_of[F.shk[k].cls] : shade_entries;
            T.gb_sh[k] = clamp_grid((shade_entries_k + per - 1) / per, F.shk[k].max_blocks);
            total_waves += (unsigned long long)T.gb_sh[k] * F.shk[k].wpb;
        }
        const double most = (double)(C.K.room_set ? (long long)(0.9 * (double)T.W.act_room) : STREAM_ACT_STATIC(T.W.cap) - 64 * (long long)total_waves) /
                            (double)(total_waves ? total_waves : 1ull);
        const double rays_in = T.b == 0 ? (double)T.nb : (double)T.n_in;
        // the shading finishes most rays' next segment itself: the list is sized for the rays measured to be left, in short chunks --
        // k_s_bounce walks every entry reserved, used or not
        const bool few_left = C.SP0.ahead && T.b < STREAM_RATE_BOUNCES && E.rate_left[T.b] >= 0.0;
        long long base = 0;
        for (int k = 0; k < F.D.n_shk; ++k) {
            const unsigned long long waves = (unsigned long long)T.gb_sh[k] * F.shk[k].wpb;
            unsigned chunk = SQ_CHUNK;
            if (act_expected >= 0.0) {
                double ex = act_expected;
                const int c = F.shk[k].cls;
                if (c >= 0 && T.b < STREAM_RATE_BOUNCES && E.rate_cls[T.b][c] >= 0.0 && E.rate_cls[T.b][c] * rays_in < ex) ex = E.rate_cls[T.b][c] * rays_in;
                if (few_left && E.rate_left[T.b] * rays_in < ex) ex = E.rate_left[T.b] * rays_in;
                if (C.split_rays) ex *= 2.0;        // (two entries per hit)
                double cc = 1.1 * ex / (double)waves + (few_left ? 48.0 : 128.0);
                if (cc > most) cc = most;
                chunk = ((unsigned)cc + 63u) & ~63u;
                if (chunk < (few_left ? 64u : (unsigned)SQ_CHUNK)) chunk = few_left ? 64u : (unsigned)SQ_CHUNK;
            }
            T.chunk_act_sh[k] = chunk;
            T.act_base_sh[k] = base;
            base += (long long)waves * (long long)chunk;
        }
        T.SP.chunk_act = T.chunk_act_sh[0];
        // the second rays' slots: at most one per ray that enters the bounce, in chunks that leave little of the ray table unused
        T.chunk_slot_sh = SQ_CHUNK;
        if (C.split_rays && total_waves) {
            double cc = 1.1 * rays_in / (double)total_waves + 64.0;
            if (cc > (double)SQ_CHUNK_MAX) cc = (double)SQ_CHUNK_MAX;
            T.chunk_slot_sh = ((unsigned)cc + 63u) & ~63u;
        }
    }
    T.gb_gen = grid_for(F.g_gen, 256 * SW_ITEMS);
    T.gb_wide = grid_for(F.g_wide, 256 * SW_ITEMS);
    T.gb_walk = grid_for(F.walk.max_blocks, SW_THREADS * SW_ITEMS);
    // the largest launches reserve 1024 (walkers) / 512 (candidates) entries per atomic: the counters are single words
    T.SP.chunk_q1 = work >= (1ll << 22) ? SQ_CHUNK_MAX : SQ_CHUNK;
    T.SP.chunk_q3 = work >= (1ll << 22) ? 512u : SQ_CHUNK;
    T.SP.static_first = C.K.static_chunks;
    T.SP.bounce_no = T.b;
    T.SP.static_general = C.K.static_chunks && !T.fresh;      // few rays behind k_s_cull: their kernels reserve as they go
    T.SP.q3_gen_chunk0 = (T.SP.static_general && T.b > 0) ? (long long)T.gb_walk * (SW_THREADS / 64) : -1;
    T.SP.gen_list = T.fresh ? T.SP.W.gen_list : nullptr;
    T.SP.slot_base0 = T.fresh ? (long long)T.gb_fresh * (sf_threads / 64) * (long long)T.SP.chunk_slot : 0;
    T.SP.hit_base0 = T.fresh ? (long long)T.gb_fresh * (sf_threads / 64) * (long long)T.SP.chunk_hit
                             : (T.fused ? (long long)T.gb_bounce * (sb_threads / 64) * (long long)T.SP.chunk_hit : 0);
}

static int launch_kernel(const StreamKernel &k, unsigned grid, StreamParams &SP, hipStream_t stream) {
    void *args[] = {(void *)&SP};
    HIP_TRY(hipLaunchKernel(k.fn, dim3(grid), dim3(k.threads), args, k.lds, stream));
    return TRC_OK;
}

// the kernels of one bounce of a slot's batch, followed by the read-back of its counters
static int launch_bounce(StreamCall &C, StreamSlot &T) {
    const StreamForms &F = C.F;
    StreamParams &SP = T.SP;
    SP.act_out = SP.W.act[T.cur];
    if (T.fresh) {
        CullParams CP;
        CP.F = SP.fp.P; CP.mask = SP.fp.mask; CP.seed = SP.P.seed; CP.rid0 = SP.P.ray_offset + (unsigned long long)T.base; CP.nb = T.nb;
        CP.fq_ray = SP.W.fq_ray; CP.fq_cell = SP.W.fq_cell; CP.gen_list = SP.W.gen_list; CP.cnt = SP.W.cnt;
        CP.room = SP.W.room; CP.chunk = T.cull_chunk; CP.gen_chunk = T.cull_gen_chunk; CP.static_first = SP.static_first;
        CP.mask_words = SP.fp.P.M * SP.fp.P.M / 32; CP.lu = CP.lv = 0; CP.gen_on = 0; CP.gen_thr = 0u;
        if (T.umask) {
            const CullParams &U = F.cull_up;
            CP.mask = U.mask; CP.mask_words = U.mask_words; CP.lu = U.lu; CP.lv = U.lv; CP.gen_on = U.gen_on; CP.gen_thr = U.gen_thr;
        }
        const StreamKernel &cull = T.umask ? F.cull_u : F.cull;
        void *cargs[] = {(void *)&CP};
        HIP_TRY(hipLaunchKernel(cull.fn, dim3(T.gb_cull), dim3(cull.threads), cargs, cull.lds, T.stream.get()));
        // (plan_bounce chose between the two-phase form and k_s_fresh, and with it k_s_cull's form)
        TRC_TRY(launch_kernel(T.fresh_one ? F.fresh_one : F.fresh, T.gb_fresh, SP, T.stream.get()));
        C.launches += 2;
    }
    if (T.fused) { TRC_TRY(launch_kernel(F.bounce, T.gb_bounce, SP, T.stream.get())); C.launches += 1; }
    if (T.first) { TRC_TRY(launch_kernel(F.first, T.gb_first, SP, T.stream.get())); C.launches += 1; }
    if (T.general) {
        TRC_TRY(launch_kernel(T.b == 0 ? F.gen0 : F.gen, T.gb_gen, SP, T.stream.get()));
        TRC_TRY(launch_kernel(F.walk, T.gb_walk, SP, T.stream.get()));
        TRC_TRY(launch_kernel(F.exact, T.gb_wide, SP, T.stream.get()));
        C.launches += 3;
    }
    if (F.D.multi) { TRC_TRY(launch_kernel({(const void *)k_s_partition, 256, 0, F.g_wide}, T.gb_part, SP, T.stream.get())); C.launches += 1; }
    for (int k = 0; k < F.D.n_shk; ++k) {
        const StreamShadeK &K = F.shk[k];
        StreamParams SK = SP;
        SK.shade_cls = K.cls;
        if (F.D.multi) {
            SK.hl_slot = SP.W.pl_slot[K.cls]; SK.hl_surf = SP.W.pl_surf[K.cls]; SK.hl_t = SP.W.pl_t[K.cls]; SK.hl_room = SP.W.pl_room; SK.hl_cn = CN(CW_CLS_LIST + K.cls);
        } else {
            SK.hl_slot = SP.W.hit_slot; SK.hl_surf = SP.W.hit_surf; SK.hl_t = SP.W.hit_t; SK.hl_room = SP.W.room; SK.hl_cn = CN(CW_HIT_LIST);
        }
        SK.chunk_act = T.chunk_act_sh[k];
        SK.act_base0 = T.act_base_sh[k];
        if (C.split_rays) SK.chunk_slot = T.chunk_slot_sh;
        SK.lds_tables = K.lds_tables; SK.lds_extra = K.lds_tables; SK.lds_fm_bins = K.lds_fm_bins;
        void *args[] = {(void *)&SK};
        HIP_TRY(hipLaunchKernel(K.fn, dim3(T.gb_sh[k]), dim3(K.threads), args, K.lds, T.stream.get()));
        C.launches += 1;
    }
    if (T.fused && SP.split_terminal == 1) {
        TRC_TRY(launch_kernel(F.absorb, clamp_grid(((long long)T.n_act + SA_THREADS * 2 - 1) / (SA_THREADS * 2), F.absorb.max_blocks), SP, T.stream.get()));
        C.launches += 1;
    }
    HIP_TRY(hipMemcpyAsync(T.h_cnt.get(), SP.W.cnt, CN_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, T.stream.get()));
    HIP_TRY(hipEventRecord(T.done.get(), T.stream.get()));
    return TRC_OK;
}

// plans the slot's next bounce and uploads its counters: everything zero except the length of the active list and, with
// pre-assigned chunks, where each list starts
static int upload_counters(const StreamCall &C, StreamSlot &T) {
    const StreamForms &F = C.F;
    plan_bounce(C, T);
    unsigned long long *up = T.h_cnt.get() + CN_WORDS;
    for (int i = 0; i < CN_WORDS; ++i) up[i] = 0ull;
    up[CN(CW_ACT_IN)] = T.n_act;
    if (T.SP.static_first) {       // the first chunk of every appending wave is pre-assigned: the lists start behind them
        // (a kernel that is not launched never closes its pre-assigned chunks: it must not be given any)
        const unsigned long long cull_waves = T.fresh ? (unsigned long long)T.gb_cull * (SC_THREADS / 64) : 0ull;
        const bool sg = T.SP.static_general != 0 && T.general;
        if (sg) {
            up[CN(CW_Q1)] = (unsigned long long)T.gb_gen * 4ull * T.SP.chunk_q1;                           // Q1 <- k_s_gen
            up[CN(CW_Q3)] = ((unsigned long long)T.gb_walk * (unsigned long long)(SW_THREADS / 64) +
                         (T.SP.q3_gen_chunk0 >= 0 ? (unsigned long long)T.gb_gen * 4ull : 0ull)) * T.SP.chunk_q3;   // Q3 <- k_s_walk (+ k_s_gen<false>)
        }
        const unsigned long long first_entries = T.first ? (unsigned long long)T.gb_first * (F.first.threads / 64) * T.SP.chunk_first : 0ull;
        up[CN(CW_HIT_LIST)] = (unsigned long long)T.SP.hit_base0 + (sg ? (unsigned long long)T.gb_wide * 4ull * SQ_CHUNK : 0ull) + first_entries;   // hit list <- k_s_fresh / k_s_bounce, k_s_exact / k_s_bounce<FRESH>
        for (int c = 0; c < TRC_CLS_COUNT; ++c) up[CN(CW_CLS_LIST + c)] = T.part_start[c];                      // class lists <- k_s_partition
        unsigned long long a = 0;                                                                      // active list <- the shading kernels
        for (int k = 0; k < F.D.n_shk; ++k) a += (unsigned long long)T.gb_sh[k] * F.shk[k].wpb * T.chunk_act_sh[k];
        up[CN(CW_ACT_OUT)] = a;
        up[CN(CW_SLOTS)] = (unsigned long long)T.SP.slot_base0 + ((sg && T.b == 0) ? (unsigned long long)T.gb_gen * 4ull * SQ_CHUNK : 0ull) + first_entries;   // slots <- k_s_fresh, k_s_gen<true> / k_s_bounce<FRESH>
        up[CN(CW_GEN_LIST)] = cull_waves * (unsigned long long)T.cull_gen_chunk;                                 // general-path list <- k_s_cull
        up[CN(CW_FP_LIST)] = cull_waves * (unsigned long long)T.cull_chunk;                                   // footprint list <- k_s_cull
        if (T.fused && T.SP.split_terminal == 1) up[CN(CW_TERM_LIST)] = (unsigned long long)T.gb_bounce * (unsigned long long)(F.bounce.threads / 64) * T.SP.chunk_thit;   // terminal hits <- k_s_bounce
    }
    // (slots are never recycled where rays split: the shading kernel goes on from the slots handed out so far)
    if (C.split_rays && T.b > 0) up[CN(CW_SLOTS)] = T.slots_used;
    HIP_TRY(hipMemcpyAsync(T.SP.W.cnt, up, CN_WORDS * sizeof(unsigned long long), hipMemcpyHostToDevice, T.stream.get()));
    return TRC_OK;
}

// ---- a call whose optics split rays: a ray table that grows --------------------------------------------------------------------
// Larger tables for a slot between two bounces: ray table, the tables beside it (streams, spectra) and every list of `room` entries,
// new_room entries each; the two active lists, new_act entries each.  What is live at that point is copied -- the records and
// streams of the slots handed out, their spectra (sample-major, `room` apart: one strided copy), the active list coming in --
// everything else of that size is scratch between bounces.  The slot's stream is idle (its last bounce has been read back).
static int split_grow(StreamSlot &T, long long new_room, long long new_act, int n_spec) {
    StreamBuffers &W = T.W;
    hipStream_t st = T.stream.get();
    const size_t live = (size_t)T.slots_used;
    auto fail = [&](int e) { T.W = StreamBuffers(); T.spec_len = 0; T.rid_len = 0; return e; };       // (a workspace half grown claims nothing)
    if (new_room > W.room) {
        DevBuf<SRayGeo> geo;
        DevBuf<SRayAux> aux;
        DevBuf<unsigned long long> rid;
        DevBuf<double> spec;
        if (int e = geo.alloc((size_t)new_room)) return fail(e);
        if (int e = aux.alloc((size_t)new_room)) return fail(e);
        if (int e = rid.alloc((size_t)new_room)) return fail(e);
        if (T.spec_on) if (int e = spec.alloc((size_t)n_spec * (size_t)new_room)) return fail(e);
        hipError_t he = hipSuccess;
        if (live) {
            he = hipMemcpyAsync(geo.get(), W.geo.get(), live * sizeof(SRayGeo), hipMemcpyDeviceToDevice, st);
            if (he == hipSuccess) he = hipMemcpyAsync(aux.get(), W.aux.get(), live * sizeof(SRayAux), hipMemcpyDeviceToDevice, st);
            if (he == hipSuccess) he = hipMemcpyAsync(rid.get(), T.rid.get(), live * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
            if (he == hipSuccess && T.spec_on)
                he = hipMemcpy2DAsync(spec.get(), (size_t)new_room * 8, T.spec.get(), (size_t)W.room * 8, live * 8, (size_t)n_spec, hipMemcpyDeviceToDevice, st);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(st);       // (the old tables go back to the pool below)
        if (he != hipSuccess) { (void)fail(TRC_ERR_DEVICE); return trc_fail(TRC_ERR_DEVICE, "copy into the grown ray table failed: %s", hipGetErrorString(he)); }
        W.geo = std::move(geo); W.aux = std::move(aux); T.rid = std::move(rid); T.rid_len = new_room;
        if (T.spec_on) { T.spec = std::move(spec); T.spec_len = (long long)n_spec * new_room; }
        const size_t cq = (size_t)new_room;
        int e = W.q1_slot.alloc(cq);
        if (!e) e = W.q1_a.alloc(cq);
        if (!e) e = W.q1_b.alloc(cq);
        if (!e) e = W.hit_slot.alloc(cq);
        if (!e) e = W.hit_surf.alloc(cq);
        if (!e) e = W.hit_t.alloc(cq);
        if (!e) e = W.gen_list.alloc(cq);
        if (!e) e = W.fq_ray.alloc(cq);
        if (!e) e = W.fq_cell.alloc(cq);
        if (e) return fail(e);
        // (the class lists of k_s_partition follow `room`: a later call that parts its hit list makes them again)
        for (int c = 0; c < TRC_CLS_COUNT; ++c) { W.pl_slot[c].reset(); W.pl_surf[c].reset(); W.pl_t[c].reset(); }
        W.pl_room = 0;
        W.room = new_room;
    }
    if (new_act > W.act_room) {
        const int in = T.cur ^ 1;           // (the list coming in, once a bounce has been shaded)
        DevBuf<uint32_t> a0, a1;
        if (int e = a0.alloc((size_t)new_act)) return fail(e);
        if (int e = a1.alloc((size_t)new_act)) return fail(e);
        if (T.b > 0 && T.n_act) {
            hipError_t he = hipMemcpyAsync((in == 0 ? a0 : a1).get(), W.act[in].get(), (size_t)T.n_act * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
            if (he == hipSuccess) he = hipStreamSynchronize(st);
            if (he != hipSuccess) { (void)fail(TRC_ERR_DEVICE); return trc_fail(TRC_ERR_DEVICE, "copy into the grown active list failed: %s", hipGetErrorString(he)); }
        }
        W.act[0] = std::move(a0); W.act[1] = std::move(a1);
        W.act_room = new_act;
    }
    return TRC_OK;
}

// Before the search kernel of a bounce of such a call: what the bounce as planned can ask of the ray table and of the lists
// (trc_split_room_need, trc_bounds.h) against what the slot has; when short, tables of at least twice the size (trc_split_grow).
// Larger tables allow larger chunks, so the bounce is planned again behind every growth.
static int split_ensure_room(const StreamCall &C, StreamSlot &T) {
    const StreamForms &F = C.F;
    for (int round = 0; round < 8; ++round) {
        plan_bounce(C, T);
        const unsigned long long live = T.b == 0 ? (unsigned long long)T.nb : (unsigned long long)T.n_in;
        const unsigned long long w_fresh = T.fresh ? (unsigned long long)T.gb_fresh * (unsigned long long)(F.fresh.threads / 64) : 0ull;
        const unsigned long long w_fused = T.fused ? (unsigned long long)T.gb_bounce * (unsigned long long)(F.bounce.threads / 64) : 0ull;
        const unsigned long long w_first = T.first ? (unsigned long long)T.gb_first * (unsigned long long)(F.first.threads / 64) : 0ull;
        const unsigned long long w_cull = T.fresh ? (unsigned long long)T.gb_cull * (SC_THREADS / 64) : 0ull;
        const unsigned long long w_gen = T.general ? (unsigned long long)T.gb_gen * 4ull : 0ull, w_exact = T.general ? (unsigned long long)T.gb_wide * 4ull : 0ull;
        // the lists of `room` entries, each with the unused tails of the waves that append to it: hit list, walker queue, k_s_cull's two
        const unsigned long long t_hit = w_fresh * T.SP.chunk_hit + w_fused * T.SP.chunk_hit + w_first * T.SP.chunk_first + w_exact * SQ_CHUNK;
        const unsigned long long t_q1 = w_gen * T.SP.chunk_q1;
        const unsigned long long t_cull = w_cull * ((unsigned long long)T.cull_chunk + T.cull_gen_chunk + SC_GEN_CAP);
        unsigned long long tails = t_hit > t_q1 ? t_hit : t_q1;
        if (t_cull > tails) tails = t_cull;
        // bounce 0: the search stage hands out the slots, at most one per ray and a chunk per wave unused
        const unsigned long long slots = T.b > 0 ? T.slots_used
                                                 : trc_split_slots_bounce0((unsigned long long)T.nb, w_fresh * T.SP.chunk_slot + w_gen * SQ_CHUNK + w_first * T.SP.chunk_first);
        const unsigned long long w_shade = (unsigned long long)T.gb_sh[0] * F.shk[0].wpb;
        const trc_split_room need = trc_split_room_need(slots, live, tails, w_shade, T.chunk_slot_sh, T.chunk_act_sh[0]);
        if ((long long)need.room <= T.W.room && (long long)need.act_room <= T.W.act_room && need.room < (1ull << 62) && need.act_room < (1ull << 62)) return TRC_OK;
        const unsigned long long new_room = trc_split_grow((unsigned long long)T.W.room, need.room), new_act = trc_split_grow((unsigned long long)T.W.act_room, need.act_room);
        if (new_room >= (unsigned long long)SQ_INVALID || new_act >= (1ull << 40))
            return trc_fail(TRC_ERR_CAPACITY, "the ray table of a call that splits rays cannot grow beyond 2^32 slots (%llu needed): slots are not recycled", need.room);
        TRC_TRY(split_grow(T, (long long)new_room, (long long)new_act, C.SP0.carry.n_spec));
        T.SP.W = T.W.view();
        T.SP.carry.slot_spec = T.spec_on ? T.spec.get() : nullptr;
        T.SP.carry.slot_rid = T.rid.get();
        if (T.b > 0) T.SP.act_in = T.SP.W.act[T.cur ^ 1];
    }
    return trc_fail(TRC_ERR_CAPACITY, "the room of a call that splits rays did not settle (%lld slots, %lld active entries)", T.W.room, T.W.act_room);
}

static int start_batch(StreamCall &C, StreamSlot &T, long long base) {
    const long long n = C.SP0.P.n;
    T.base = base;
    T.nb = (n - base < C.cap) ? (n - base) : C.cap;
    T.n_in = T.nb; T.n_act = 0; T.b = 0; T.cur = 0; T.attempt = 0; T.busy = true;
    T.slots_used = 0;
    T.SP = C.SP0;
    T.SP.W = T.W.view();
    T.SP.carry.slot_spec = T.spec_on ? T.spec.get() : nullptr;
    T.SP.carry.slot_rid = C.split_rays ? T.rid.get() : nullptr;
    T.SP.base = base;
    T.SP.nb = T.nb;
    if (C.split_rays) TRC_TRY(split_ensure_room(C, T));
    TRC_TRY(upload_counters(C, T));
    return launch_bounce(C, T);
}

// called when the slot's last launch has completed: takes in its counters and launches its next bounce, if any
static int advance(StreamCall &C, StreamSlot &T) {
    StreamEngine &E = C.E;
    const unsigned long long *c = T.h_cnt.get();
#ifdef SW_STATS
    if (T.fresh) fprintf(stderr, "batch %lld: footprint list %llu entries of %lld rays (%s)\n", T.base / C.cap, c[CN(CW_FP_LIST)], T.nb, T.umask ? "umask" : "Cartesian mask");
    fprintf(stderr, "batch %lld bounce %d: Q1 %llu Q3 %llu hits %llu | walkers %llu wave-iters %llu steps %llu leaf-entries %llu box-tests %llu drains %llu drain-rounds %llu\n",
            T.base / C.cap, T.b, c[CN(CW_Q1)], c[CN(CW_Q3)], c[CN(CW_HITS)], c[CN(CW_STATS)], c[CN(CW_STATS + 1)], c[CN(CW_STATS + 2)], c[CN(CW_STATS + 3)], c[CN(CW_STATS + 4)], c[CN(CW_STATS + 5)], c[CN(CW_STATS + 6)]);
#endif
    if (c[CN(CW_OVERFLOW)]) {
        // The candidate queue was too small for this bounce.  Nothing of the bounce has been committed (k_s_exact,
        // k_s_shade returns at once when the flag is set): double the queue and run the bounce again.
        if (c[CN(CW_OVERFLOW)] != CW_OVF_RETRY || T.attempt >= 6) return trc_fail(TRC_ERR_CAPACITY, "streaming queues overflow (%llu candidate pairs, capacity %lld)", c[CN(CW_Q3)], T.W.q3_cap);
        ++T.attempt;
        TRC_TRY(T.W.grow_q3());
        T.SP.W = T.W.view();
        TRC_TRY(upload_counters(C, T));
        return launch_bounce(C, T);
    }
    T.attempt = 0;
    if (C.split_rays) T.slots_used = c[CN(CW_SLOTS)];       // (reserved: the unused tails of the waves' chunks stay unused)
    // The rays whose next segment this bounce's shading finished itself (StreamParams.ahead): a segment each of the bounce they were
    // finished for, which then has run as far as they are concerned; their hits are in CW_HITS and CW_TERM_HITS, which the rates
    // below -- what the kernels of THIS bounce found -- leave out.  They are in neither CW_ALIVE nor CW_ACT_OUT.
    const unsigned long long n_ahead = c[CN(CW_AHEAD)], ahead_hits = c[CN(CW_AHEAD_HITS)];
    C.seg += (double)T.n_in + (double)n_ahead;
    C.hits += (double)c[CN(CW_HITS)];
    if (T.fresh && T.nb > 0) {       // what the next batches can expect (with a margin; a low guess only costs atomics)
        const double rate = 1.15 * (double)(c[CN(CW_HITS)] - ahead_hits) / (double)T.nb + 256.0 / (double)T.nb;
        if (rate > E.fp_hit_rate || E.fp_hit_rate > 2.0 * rate) E.fp_hit_rate = rate;
    }
    if (T.fused && T.b < STREAM_RATE_BOUNCES && T.n_in > 0) {       // (without the split CN(CW_TERM_HITS) stays 0: every hit is on the one list)
        const double nin = (double)T.n_in, pad = 512.0 / nin;
        const double rt = 1.15 * (double)(c[CN(CW_TERM_HITS)] - ahead_hits) / nin + pad, ro = 1.15 * (double)(c[CN(CW_HITS)] - c[CN(CW_TERM_HITS)]) / nin + pad;
        if (E.rate_term[T.b] < 0.0 || rt > E.rate_term[T.b] || E.rate_term[T.b] > 2.0 * rt) E.rate_term[T.b] = rt > 1.0 ? 1.0 : rt;
        if (E.rate_other[T.b] < 0.0 || ro > E.rate_other[T.b] || E.rate_other[T.b] > 2.0 * ro) E.rate_other[T.b] = ro > 1.0 ? 1.0 : ro;
    }
    if (T.b < STREAM_RATE_BOUNCES) {
        const double rin = T.b == 0 ? (double)T.nb : (double)T.n_in;
        if (rin > 0.0)
            for (int cl = 0; cl < TRC_CLS_COUNT; ++cl) {
                const double r = 1.15 * (double)c[CN(CW_CLS_HITS + cl)] / rin + 512.0 / rin;
                double &R = E.rate_cls[T.b][cl];
                if (R < 0.0 || r > R || R > 2.0 * r) R = r;
                C.cls_hits[cl] += (double)c[CN(CW_CLS_HITS + cl)];
            }
    }
    if (C.SP0.ahead && T.b < STREAM_RATE_BOUNCES) {
        const double rin = T.b == 0 ? (double)T.nb : (double)T.n_in;
        if (rin > 0.0) {
            const double r = 1.15 * (double)c[CN(CW_ALIVE)] / rin + 512.0 / rin;
            double &R = E.rate_left[T.b];
            if (R < 0.0 || r > R || R > 2.0 * r) R = r;
        }
    }
    if (T.b + 1 > C.max_bounces) C.max_bounces = T.b + 1;
    if (n_ahead && T.b + 2 > C.max_bounces) C.max_bounces = T.b + 2;
    if (c[CN(CW_ALIVE)] == 0 || T.b + 1 >= C.SP0.P.reps) { T.busy = false; return TRC_OK; }
    // next bounce: the rays just shaded are the active list
    T.n_act = c[CN(CW_ACT_OUT)];                                       // its reserved entries (the tail of the last chunks is invalid)
    T.n_in = (long long)c[CN(CW_ALIVE)];
    T.SP.act_in = T.SP.W.act[T.cur];
    T.cur ^= 1;
    T.b += 1;
    if (C.split_rays) TRC_TRY(split_ensure_room(C, T));
    TRC_TRY(upload_counters(C, T));
    return launch_bounce(C, T);
}

// Runs the whole call batch by batch, two batches in flight.  P is fully set up by trc_trace_fast (inputs staged, source uploaded),
// which has planned the search (stream_plan) and read the knobs.
static int stream_trace(trc_scene *sc, FastParams &P, const CarryIn &carry_in, const StreamPlan &plan, trc_facts &facts, const trc_source_desc *src_desc,
                        StreamEngine &E, trc_trace_stats *stats, double *seg_out, double *hit_out) {
    trc_ctx *ctx = sc->ctx;
    const StreamKnobs &K = facts.knobs;
    // Batches: equal parts, a multiple of the number of slots (so that the slots finish together), at most 2^26 rays each
    // (14 GB of workspace per slot); calls below 2^23 rays are not split.
    const long long cap_max = 1ll << 26;
    int n_slots = (P.n >= (1ll << 23)) ? K.slots : 1;
    long long n_batches = n_slots * ((P.n + n_slots * cap_max - 1) / (n_slots * cap_max));
    long long cap = (P.n + n_batches - 1) / n_batches;
    cap = (cap + 63) & ~63ll;
    if (cap < 64) cap = 64;
    TRC_TRY(stream_engine_init(&E, ctx));
    if (E.rate_geom_version != sc->search.geom_version()) {       // another pose of the scene: measured again
        E.forget_rates();
        E.rate_geom_version = sc->search.geom_version();
    }
    // rays that carry more than the fast engine's record -- Im of a complex index, materials at their wavelength, a spectrum -- are
    // shaded by k_s_shade_x; the spectra of the rays under way live in a table of their own beside the ray table
    // ... and so are all hits of a scene whose optics send two rays on from a hit, by its SPLIT form
    const bool split_rays = sc->surfaces.splits();
    facts.call.carry = sc->surfaces.needs().any() || carry_in.ref_im || carry_in.mat || carry_in.spec || split_rays || facts.call.poly_src > 0;
    StreamForms F;
    StreamCall C{F, K, E, StreamParams(), cap, 0.0, 0.0, {0.0, 0.0, 0.0}, 0, 0, split_rays};
    memset(&C.SP0, 0, sizeof(C.SP0));
    C.SP0.P = P;
    C.SP0.carry = carry_in;
    TRC_TRY(stream_choose_forms(F, C.SP0, sc, E, plan, facts, src_desc));
    TRC_TRY(stream_slots_alloc(E, n_slots, cap, sc, carry_in, F, K, split_rays, facts.call.poly_src > 0));

    for (int k = 0; k < STREAM_MAX_SLOTS; ++k) E.slot[k].busy = false;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int k = 1; k < n_slots; ++k) HIP_TRY(hipStreamWaitEvent(E.slot[k].stream.get(), ctx->ev0, 0));   // inputs were staged on the context's stream
    long long next_base = 0;
    int turn = 0;
    int rc = TRC_OK;
    for (;;) {
        for (int k = 0; k < n_slots && rc == TRC_OK; ++k)
            if (!E.slot[k].busy && next_base < P.n) { rc = start_batch(C, E.slot[k], next_base); next_base += cap; }
        if (rc != TRC_OK) break;
        int n_busy = 0;
        for (int k = 0; k < n_slots; ++k) n_busy += E.slot[k].busy ? 1 : 0;
        if (!n_busy) break;
        // serve a slot whose launch is complete; if none is, wait for the next busy one in turn
        int k = -1;
        for (int j = 0; j < n_slots; ++j) {
            const int q = (turn + j) % n_slots;
            if (!E.slot[q].busy) continue;
            if (k < 0) k = q;
            if (hipEventQuery(E.slot[q].done.get()) == hipSuccess) { k = q; break; }
        }
        hipError_t se = hipEventSynchronize(E.slot[k].done.get());
        if (se != hipSuccess) { rc = trc_fail(TRC_ERR_DEVICE, "streaming bounce failed: %s", hipGetErrorString(se)); break; }
        rc = advance(C, E.slot[k]);
        if (rc != TRC_OK) break;
        turn = (k + 1) % n_slots;
    }
    // drain both streams whatever happened, then close the timed region on the context's stream
    for (int k = 0; k < n_slots; ++k) (void)hipStreamSynchronize(E.slot[k].stream.get());
    if (rc != TRC_OK) {
        // what the bounces that did complete have added to the private tallies must not reach the scene with a later call; the
        // caller (trc_trace_fast) winds the hit buffer back, which leaves the chunks they opened in it stale
        for (int k = 0; k < n_slots; ++k)
            if (E.slot[k].W.tally_part) (void)hipMemset(E.slot[k].W.tally_part.get(), 0, (size_t)TALLY_PARTS * (size_t)E.slot[k].W.tally_n * sizeof(double));
        return rc;
    }
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float total_ms = 0;
    (void)hipEventElapsedTime(&total_ms, ctx->ev0, ctx->ev1);
    for (int k = 0; k < n_slots; ++k)
        hipLaunchKernelGGL(k_s_merge_tallies, dim3((unsigned)((sc->tally.size() + 255) / 256)), dim3(256), 0, ctx->stream, sc->tally.device(), E.slot[k].W.tally_part.get(), (long long)sc->tally.size());
    hipLaunchKernelGGL(k_s_add2, dim3(1), dim3(64), 0, ctx->stream, sc->tally.device() + 3 * sc->n_surf, C.seg, C.hits);
    // (not waited for: whatever reads or resets the tallies synchronises the context's stream first, and the next call's kernels
    // are ordered behind these by ev0)
    stats->kernel_ms = total_ms;
#ifdef SB_STATS
    {
        unsigned long long h[32];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_sb_stats), sizeof(h)) == hipSuccess) {
            for (int f = 0; f < 2; ++f) {
                const unsigned long long *q = h + 16 * f;
                const double nr = q[7] ? (double)q[7] : 1.0, nw = q[9] ? (double)q[9] : 1.0;
                fprintf(stderr, "k_s_bounce, %s rays: %llu in %llu wave passes; per ray: cells %.2f (occupied %.2f), entries %.2f, passed %.2f, exact tests %.2f; "
                                "per wave pass: walk turns %.1f, rounds of exact tests %.1f\n", f ? "continued" : "fresh", q[7], q[9], q[0] / nr, q[4] / nr, q[1] / nr,
                        q[2] / nr, q[3] / nr, q[5] / nw, q[6] / nw);
                if (f) fprintf(stderr, "k_s_bounce, continued rays inside a clear cone (no walk): %llu\n", q[10]);
            }
            memset(h, 0, sizeof(h));
            hipMemcpyToSymbol(HIP_SYMBOL(g_sb_stats), h, sizeof(h));
        }
    }
#endif
    stats->launches = C.launches + 1;
    stats->bounces = C.max_bounces;
    *seg_out = C.seg;
    *hit_out = C.hits;
    return TRC_OK;
}
