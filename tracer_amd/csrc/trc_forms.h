// trc_forms.h -- which kernel instance every engine runs for a call, decided from plain numbers.
//
// The library holds some 140 instances of its search, shading, megakernel and ordered-bounce kernels, and picks among them per call by
// arithmetic on the sizes of the scene and the call's flags.  That arithmetic lives here, free of HIP: FACTS (what the decisions
// read), DECISIONS (every per-call choice the host drivers make, each stage with its kernel id -- family and template arguments as
// integers -- its threads and its bytes of dynamic LDS) and trc_kernel_name (an id as a kernel trace spells it).  The host drivers
// (trc_stream.inc, trc_kernels.hip) gather the facts, decide here, and turn each id into a function pointer in one place per family
// that reads nothing but the id.  tests/hostcheck compiles this header with g++ and holds the restatements of tests/*_cases.py to it.
// Every threshold of the choice is named here, once, beside the decision that compares with it.
#ifndef TRC_FORMS_H
#define TRC_FORMS_H

#include <cstdio>
#include "trc_bounds.h"
#include "trc_footprint.h"

// ------------------------------------------------------------------------------------------------
// launch shapes and per-wave LDS blocks the kernels are built for (the kernels read the same macros)
// ------------------------------------------------------------------------------------------------
#define SC_THREADS 512                  /* k_s_cull, k_s_ucull */
#define SC_GEN_CAP 1024                 /* general-path rays a workgroup of k_s_cull collects before it appends them */
// k_s_fresh, k_s_fresh2: one workgroup per CU: 1024 threads (4 waves per SIMD) for a scene of flat surfaces -- 128 registers with 18
// of the instance's 160 in scratch, and still a quarter faster than 3 waves per SIMD without (NSTTF: 0.33 -> 0.25 ms per batch: the
// kernel issues at half the rate of its arithmetic, its dependent float64 chains want waves to switch to) -- 512 (2 per SIMD) with the
// quadric code in; every table then exists once per CU
#define SF_THREADS(FLAT) ((FLAT) ? 1024 : 768)
#define SF2_DERIVES_CELL(FLAT, LDS) ((FLAT) || (LDS))   /* the instances of k_s_fresh2 that find the list cell of a ray themselves */
#ifndef SW_LEAFCAP
#define SW_LEAFCAP 16
#endif
#ifndef SW_LIST_T
#define SW_LIST_T uint16_t
#endif
#ifndef SW_THREADS
#define SW_THREADS 256
#endif
#define SB_THREADS 1024          /* one workgroup per CU, 4 waves per SIMD: every table exists once per CU.  The instances with the quadric
                                    code in need ~166 registers and keep 18 of them in scratch at 128 (dish + receiver: 19.7 -> 18.3 ms per
                                    1e8 rays against 768 threads; the seven-wall cavity: unchanged); the flat instance needs 121 */
#define SB_THREADS_OF(GRIDM) (SB_THREADS)       /* (768 and 512 threads on the large grid, no scratch then: 16.3 and 21.2 ms against 14.2 per 1e7 rays on the relief) */
#define SA_THREADS 1024          /* k_s_absorb */
#ifndef SHC_THREADS
#define SHC_THREADS 1024         /* k_s_shade_c, k_s_shade_x */
#endif
#define SH_THREADS 256           /* k_s_shade<.., 2, ..>: 128 threads per wave of a SIMD it is built for */
#define COOP_LEAFCAP 16      // k_trace_coop: leaves listed per lane between two drains
#define COOP_E 128           // exact-test queue entries per wave
#define COOP_FIXED_BYTES (COOP_E * 8 + 64 * 8 + COOP_E * 4 + 64 * 4 + 64 * 4 + 64 * 4 + COOP_LEAFCAP * 64 * 2)
// a wave's block of k_trace_coop / of k_s_walk: its queues and lists, and DEPTH rows of its packed stack.  (Macros, as the kernels
// have always read them: as inline functions the same arithmetic moved k_trace_coop's register allocation -- 165 -> 167 registers.)
#define COOP_WAVE_BYTES(DEPTH) ((size_t)(DEPTH) * 64 * 4 + COOP_FIXED_BYTES)
#define SW_WAVE_BYTES(DEPTH) ((size_t)(DEPTH) * 64 * 4 + SW_LEAFCAP * 64 * sizeof(SW_LIST_T) + 64 * 4)

// ------------------------------------------------------------------------------------------------
// thresholds
// ------------------------------------------------------------------------------------------------
// dynamic LDS a workgroup may ask for: of the CU's 160 KiB once allowed them (kernel_allow_lds; 512 bytes stay with the kernels'
// static LDS), and what any kernel gets unasked (k_trace_fast keeps to it)
static const size_t LDS_MAX_ALLOWED = 160 * 1024 - 512;
static const size_t LDS_MAX_PLAIN = 64 * 1024;
static const size_t TRC_SEARCH_LDS_LIMIT = 150 * 1024;     // up to here the tables of k_s_fresh / k_s_bounce go to LDS
static const size_t TRC_EXACT_RECS_LIMIT = 40 * 1024;      // ... and the surface records of k_s_exact
static const long long TRC_FP_LIST_LIMIT = 65536;          // a footprint list in LDS holds 16-bit offsets: fewer entries than this
#define TRC_MAX_SURFACES16 65535        /* the packed structures (Kd leaves, the list of all boxes) hold 16-bit surface numbers */
#define STREAM_SMALL_SURFACES 24        /* scenes up to this many surfaces take their fresh rays through k_s_bounce<.., FRESH> */
#define STREAM_TINY_SURFACES 4          /* ... and up to this many are searched surface by surface (k_s_bounce<3>) */
#define TRC_BG_OCC_COOP_BYTES (80 * 1024)       /* occupancy bits of the large grid in LDS: beside k_s_bounce_coop's blocks */
#define TRC_BG_OCC_LANES_BYTES (96 * 1024)      /* ... and in k_s_bounce<2> */
#define COOP_MAX_NODES 16384    // k_trace_coop: stack entries are 4 bytes: node (14 bits) | axis code (2 bits) | interval end (16 bits)
#define COOP_MAX_DEPTH 24
#define ORD_STACK_DEPTH 24      // k_ord_bounce<1>: entries of a thread's stack in LDS
#define TRC_STREAM_MIN_RAYS 1048576     /* calls from this many rays on run the streaming engine */
#define TRC_STREAM_MIN_RAYS_BIG 4096    /* ... from this many in a scene on the large grid */
#define TRC_STREAM_FEWEST_RAYS 64       /* ... and no call below this many, whatever its flags */

// ------------------------------------------------------------------------------------------------
// classes of surfaces
// ------------------------------------------------------------------------------------------------
// optics kinds of the "mirrors and diffuse walls" family: what a heliostat field, a dish or a cavity of opaque walls is made of.
// A scene of flat surfaces with only these gets an instance of k_s_shade that carries nothing else (SIMPLE).
#define TRC_OPT_SIMPLE_MASK ((1u << TRC_OPT_TRANSPARENT) | (1u << TRC_OPT_REFLECTIVE) | (1u << TRC_OPT_ONE_SIDED_REFLECTIVE) | \
                             (1u << TRC_OPT_REAL_REFLECTIVE) | (1u << TRC_OPT_ONE_SIDED_REAL_REFLECTIVE) | (1u << TRC_OPT_LAMBERTIAN) | \
                             (1u << TRC_OPT_LAMBERTIAN_SPECULAR))
// The shading kernel that serves a surface (trc_shade.hip): the lean kernels take the optics that need a handful of registers (eight
// waves per SIMD and more); everything else -- refraction, media, conductors, incidence-angle modifiers -- by k_s_shade.
#define TRC_CLS_MIRROR 0       /* Transparent, Reflective, OneSidedReflective, RealReflective, OneSidedRealReflective (no IAM) */
#define TRC_CLS_DIFFUSE 1      /* Lambertian (no IAM, no absorbing medium), LambertianSpecular, SemiLambertian, Reflective_spectral, the
                                  Lambertian_directional_axisymmetric_piecewise family */
#define TRC_CLS_GENERAL 2
#define TRC_CLS_COUNT 3
#define TRC_CLS_MIRROR_KINDS ((1u << TRC_OPT_TRANSPARENT) | (1u << TRC_OPT_REFLECTIVE) | (1u << TRC_OPT_ONE_SIDED_REFLECTIVE) | \
                              (1u << TRC_OPT_REAL_REFLECTIVE) | (1u << TRC_OPT_ONE_SIDED_REAL_REFLECTIVE))
#define TRC_CLS_DIFFUSE_KINDS ((1u << TRC_OPT_LAMBERTIAN) | (1u << TRC_OPT_LAMBERTIAN_SPECULAR) | (1u << TRC_OPT_SEMI_LAMBERTIAN) | \
                               (1u << TRC_OPT_REFLECTIVE_SPECTRAL) | (1u << TRC_OPT_LAMBERTIAN_DIRECTIONAL) |                     \
                               (1u << TRC_OPT_LAMBERTIAN_DIRECTIONAL_SPECTRAL) | (1u << TRC_OPT_FRESNEL_CONDUCTOR))

// class of a surface from its optics kind and parameters (host side, when the flags are uploaded)
static inline int trc_shade_class_of(const trc_surface_desc &sd) {
    const int ok = sd.optics_kind;
    if (ok < 0 || ok >= 32) return TRC_CLS_GENERAL;
    if ((TRC_CLS_MIRROR_KINDS >> ok) & 1u) {
        const bool iam = ((ok == TRC_OPT_REFLECTIVE || ok == TRC_OPT_ONE_SIDED_REFLECTIVE) && sd.opt[1] != 0.0) ||
                         ((ok == TRC_OPT_REAL_REFLECTIVE || ok == TRC_OPT_ONE_SIDED_REAL_REFLECTIVE) && sd.opt[3] != 0.0);
        return iam ? TRC_CLS_GENERAL : TRC_CLS_MIRROR;
    }
    if ((TRC_CLS_DIFFUSE_KINDS >> ok) & 1u) {
        if (ok == TRC_OPT_LAMBERTIAN && (sd.opt[2] != 0.0 || sd.opt[4] != 0.0)) return TRC_CLS_GENERAL;      // absorbing medium / IAM
        return TRC_CLS_DIFFUSE;
    }
    return TRC_CLS_GENERAL;
}

// TRC_SURF_TERMINAL: e_out = e (1 - absorptivity) = 0 exactly, and 0 <= min_energy for every min_energy the API accepts
static inline bool surface_ends_every_ray(const trc_surface_desc &sd) {
    const int ok = sd.optics_kind;
    const bool plain = ((ok == TRC_OPT_REFLECTIVE || ok == TRC_OPT_ONE_SIDED_REFLECTIVE) && sd.opt[1] == 0.0) ||
                       ((ok == TRC_OPT_REAL_REFLECTIVE || ok == TRC_OPT_ONE_SIDED_REAL_REFLECTIVE) && sd.opt[3] == 0.0) ||
                       (ok == TRC_OPT_LAMBERTIAN && sd.opt[2] == 0.0 && sd.opt[4] == 0.0) || ok == TRC_OPT_LAMBERTIAN_SPECULAR;
    return plain && sd.opt[0] == 1.0;
}

// ------------------------------------------------------------------------------------------------
// the LDS images of the search kernels, by their parts (trc_search_lds_layout, trc_bounds.h)
// ------------------------------------------------------------------------------------------------
// the footprint-listed kernels' LDS image: [the Buie table] [records | oriented boxes | cell offsets | lists (lds)] [queues]
TRC_HD trc_lds_parts fresh_lds_parts(int n_surf, int stride, const trc_fp_params &F, long long n_list, bool buie, bool lds, int queue_waves) {
    trc_lds_parts p = {};
    p.n_surf = n_surf; p.stride = stride;
    p.buie_bytes = buie ? (int)sizeof(trc_buie_fast) : 0;
    p.tables = lds;
    if (lds) { p.fp_offs = F.Mc * F.Mc + 1; p.fp_list = (int)n_list; }
    p.queue_waves = queue_waves;
    return p;
}
// the LDS image of k_s_bounce / k_s_bounce_coop: [the Buie table (fresh)] [occupancy bits] [records | oriented boxes | boxes | flags |
// small grid (lds)] [the waves' blocks (coop)]
TRC_HD trc_lds_parts bounce_lds_parts(int n_surf, int stride, bool fresh, bool lds, bool flags, int grid_cells, int grid_list, int occ_words,
                                      int coop_waves) {
    trc_lds_parts p = {};
    p.n_surf = n_surf; p.stride = stride;
    p.buie_bytes = fresh ? (int)sizeof(trc_buie_fast) : 0;
    p.occ_words = occ_words;
    p.tables = p.sbox = lds;
    p.flags = flags;
    if (grid_cells) { p.grid_cells = grid_cells; p.grid_list = grid_list; }
    p.coop_waves = coop_waves;
    return p;
}
// Dynamic LDS of a search kernel from its image: what a fits-in-LDS decision compares with its limit, and what a launch asks for -- 16
// bytes more, so that it is never 0 and a block the kernel puts behind the image can start on 16 bytes
static inline size_t lds_need(const trc_lds_layout &L) { return L.end + L.slack; }
static inline size_t lds_request(const trc_lds_layout &L) { return lds_need(L) + 16; }
static inline size_t shade_lds_need(const trc_shade_parts &p) { const trc_shade_layout L = trc_shade_lds_layout(p); return L.end + L.slack; }

// ------------------------------------------------------------------------------------------------
// FACTS
// ------------------------------------------------------------------------------------------------
// Environment knobs of the streaming engine: routes and capacities the tests compare and force.  trc_trace_fast reads them at every
// call, since the tests switch them within one process.
struct StreamKnobs {
    int search;             // TRC_STREAM_SEARCH=1: walk the caller's Kd-tree instead of the grid (when its walk kernel fits)
    bool fresh;             // TRC_STREAM_FRESH=0: no footprint map
    bool bounce;            // TRC_STREAM_BOUNCE=0: continued rays through the general path
    bool first;             // TRC_STREAM_FIRST=1: fresh rays outside the footprint map through k_s_bounce<.., FRESH>
    bool coop;              // TRC_STREAM_COOP=0: k_s_bounce<2> on the large grid, every lane its own ray
    int absorb;             // TRC_STREAM_ABSORB=0: no list of terminal hits; =1: the list, finished by k_s_absorb only (-1: not set)
    bool static_chunks;     // TRC_STREAM_STATIC=0: no pre-assigned chunks
    bool room_set; long long room;      // TRC_STREAM_ROOM is set, and the room of every list it sets (>= 64; 0: the default)
    long long q3_entries;   // TRC_STREAM_Q3_ENTRIES: initial capacity of the candidate queue (0: by the batch)
    int fp_cells;           // TRC_STREAM_FP_CELLS: cells per side of the footprint map (>= 32; 0: by the scene)
    bool umask;             // TRC_STREAM_UMASK=0: k_s_cull on the Cartesian mask for every source (the form that packs the cell)
    int slots;              // TRC_STREAM_SLOTS: batches in flight, 1 .. STREAM_MAX_SLOTS (default 2)
    bool clear = true;      // TRC_STREAM_CLEAR=0: k_s_bounce gets no table of clear cones, every continued ray walks the grid
    bool ahead = true;      // TRC_STREAM_AHEAD=0: k_s_shade_c finishes no ray's next segment, every continued ray goes to k_s_bounce
};

// What the decisions read of a scene.  Two parts: the sizes, which cost nothing to gather, and what only a pass over the surfaces
// tells (`walked`), which the streaming engine alone asks for -- a mesh of 1e5 faces pays for that pass at every call, once.
struct trc_scene_facts {
    int n_surf, stride;
    bool accel_ok, accel_kd_ok, has_kd;         // the boxes were built; the caller's Kd-tree is packed beside them; it set one
    int kd_nodes, kd_nleaf, kd_nalways, kd_depth;
    bool grid_ok, big_ok;                       // the scene stands on the LDS-sized grid / on the large one
    int grid_cells, grid_list;                  // cells and list entries of the LDS-sized grid
    int brute_list, n_unbounded;                // entries of the list of all boxes; surfaces without a box
    int big_occ_words;                          // occupancy words of the large grid
    int n_fm_edges, fms_bytes, n_extra;         // flux maps: edges of all maps, bytes of their descriptors; doubles of optics tables
    long long fm_bins;                          // bins of all flux maps
    bool chart;                                 // some flux map bins in another chart than XY
    bool transfer;                              // the transfer matrix is kept
    bool splits;                                // some optics send two rays on from a hit
    // the pass over the surfaces
    bool walked;
    bool all_flat;                              // every geometry kind is flat
    bool simple;                                // ... and every optics kind one of TRC_OPT_SIMPLE_MASK
    unsigned cls_moving, cls_all;               // bit c: class c is present among the surfaces that do not end every ray / among all
    bool any_term;                              // some surface ends every ray
    // (not part of the pass) the search tables hold clear cones (trc_clear_build); false wherever nobody says so
    bool clear_cones;
};
// what a call brings
struct trc_call_facts {
    long long n;
    int flags;                  // TRC_TRACE_*
    int src_kind;               // of the source descriptor, -1: the rays are given
    bool spec;                  // the source has a spectrum
    bool carry;                 // the rays carry more than the fast engine's record (complex indices, materials, spectra)
    bool mat_dev;               // the materials' tables are on the device and the call brings no rows of them
    bool term_ok;               // 0 <= min_energy: a ray of energy 0 ends in the reference too
    int poly_src;               // the source carries its spectrum (TRC_SPECTRUM_CARRIED): the points W of its table, 0: it does not
    int poly_walls;             // ... and the polychromatic walls of the scene, whose lambda cells k_s_shade_p may stage
};
// the footprint map of the call's source, after stream_fp_prepare
struct trc_fp_facts {
    bool use;
    long long n_list;
    int M, Mc;
    bool has_generic;
    double cdf_end, coverage, ucoverage;
    int umask_words, Mu, Mv;    // the mask over the uniforms as uploaded (0 words: none)
};
struct trc_facts { trc_scene_facts scene; trc_call_facts call; trc_fp_facts fp; StreamKnobs knobs; };

// The part of the scene facts that (surfs, accel) decide; `walk`: with the pass over the surfaces.  The caller adds what it keeps
// itself: stride, accel_ok, the Kd-tree's counts, the flux maps, transfer, splits.
static inline void trc_scene_facts_fill(const trc_surface_desc *surfs, int n_surf, const trc_accel_host &A, bool walk, trc_scene_facts *s) {
    s->n_surf = n_surf;
    s->kd_depth = A.kd_depth;
    s->grid_ok = A.grid_ok; s->big_ok = A.big_ok;
    s->grid_cells = A.grid_off.empty() ? 0 : (int)A.grid_off.size() - 1;
    s->grid_list = (int)A.grid_list.size();
    s->brute_list = (int)A.brute_leaf.size();
    s->n_unbounded = (int)A.unbounded.size();
    s->big_occ_words = (int)A.big_occ.size();
    s->clear_cones = A.clear_cones > 0;
    s->walked = walk;
    if (!walk) return;
    s->all_flat = s->simple = true;
    s->cls_moving = s->cls_all = 0u;
    s->any_term = false;
    for (int i = 0; i < n_surf; ++i) {
        const trc_surface_desc &sd = surfs[i];
        const bool flat = trc_gm_is_flat(sd.gm_kind);
        s->all_flat = s->all_flat && flat;
        s->simple = s->simple && flat && ((TRC_OPT_SIMPLE_MASK >> sd.optics_kind) & 1u);
        const unsigned bit = 1u << trc_shade_class_of(sd);
        s->cls_all |= bit;
        if (surface_ends_every_ray(sd)) s->any_term = true;
        else s->cls_moving |= bit;
    }
}

// ------------------------------------------------------------------------------------------------
// kernel ids and their names
// ------------------------------------------------------------------------------------------------
enum trc_kernel_family {
    TRC_K_NONE,                 // the call has no such stage
    TRC_K_CULL, TRC_K_UCULL,    // k_s_cull<KIND>, k_s_ucull<KIND>
    TRC_K_FRESH, TRC_K_FRESH2,  // k_s_fresh<KIND, FLAT, LDS>, k_s_fresh2<KIND, FLAT, LDS>
    TRC_K_BOUNCE,               // k_s_bounce<GRIDM, LDS, FRESH, FLAT, SUN>
    TRC_K_BOUNCE_COOP,          // k_s_bounce_coop<FRESH, FLAT, SUN>
    TRC_K_WALK,                 // k_s_walk<THREADS, GRID>
    TRC_K_GEN, TRC_K_GEN_SRC,   // k_s_gen<FRESH, KIND>, k_s_gen_src<KIND>
    TRC_K_EXACT,                // k_s_exact
    TRC_K_SHADE,                // k_s_shade<SIMPLE, WAVES, LDS, SPEC, CHART>
    TRC_K_SHADE_C,              // k_s_shade_c<CLS, FLATN, LDS, SPEC, CHART>
    TRC_K_SHADE_X,              // k_s_shade_x<LDS, CHART, SPLIT, MAT>
    TRC_K_ABSORB,               // k_s_absorb
    TRC_K_TRACE_COOP, TRC_K_TRACE_FAST,         // k_trace_coop<THREADS, SPEC, SUN, CHART>, k_trace_fast<THREADS, SPEC, SUN, CHART>
    TRC_K_ORD_BOUNCE,           // k_ord_bounce<MODE, CHART, MAT>
    TRC_K_SHADE_P,              // k_s_shade_p<LDS, CHART, SPLIT>
    // the arc-lamp sources (trc_src_kind_is_lamp): kernels of their own names, so that every instance of the families above -- their
    // names, their template arguments, their code -- stays what it was before these sources
    TRC_K_GEN_LAMP,             // k_s_gen_lamp<KIND>: k_s_gen<true, KIND>'s body for a lamp kind
    TRC_K_LAMP_COOP, TRC_K_LAMP_FAST,           // k_lamp_coop<THREADS, SPEC, CHART>, k_lamp_fast<THREADS, SPEC, CHART>: the megakernel's text (trc_mega.inc)
    // the thermal emitters (TRC_SRC_EMIT_THERMAL; with the lamps: trc_src_kind_is_emitter): a generation kernel of its own name;
    // the megakernel's instances are the lamps', whose trc_lamp_ray_t<-1> knows the kind
    TRC_K_GEN_EMIT,             // k_s_gen_emit: k_s_gen<true, TRC_SRC_EMIT_THERMAL>'s body
    TRC_K_FAMILIES
};
struct trc_kernel_id { int family; int a[5]; };     // the template arguments in their order, bool as 0 / 1; unused: 0
static inline trc_kernel_id trc_kid(int family, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0) { return {family, {a0, a1, a2, a3, a4}}; }
static inline bool trc_kid_equal(const trc_kernel_id &x, const trc_kernel_id &y) {
    return x.family == y.family && x.a[0] == y.a[0] && x.a[1] == y.a[1] && x.a[2] == y.a[2] && x.a[3] == y.a[3] && x.a[4] == y.a[4];
}

// name and argument kinds of a family: 'i' an integer, 'b' a bool
static inline const char *trc_kernel_family_name(int family, const char **args) {
    static const char *const names[TRC_K_FAMILIES][2] = {
        {"", ""}, {"k_s_cull", "i"}, {"k_s_ucull", "i"}, {"k_s_fresh", "ibb"}, {"k_s_fresh2", "ibb"}, {"k_s_bounce", "ibbbb"}, {"k_s_bounce_coop", "bbb"},
        {"k_s_walk", "ib"}, {"k_s_gen", "bi"}, {"k_s_gen_src", "i"}, {"k_s_exact", ""}, {"k_s_shade", "bibbb"}, {"k_s_shade_c", "ibbbb"},
        {"k_s_shade_x", "bbbb"}, {"k_s_absorb", ""}, {"k_trace_coop", "ibbb"}, {"k_trace_fast", "ibbb"}, {"k_ord_bounce", "ibb"},
        {"k_s_shade_p", "bbb"}, {"k_s_gen_lamp", "i"}, {"k_lamp_coop", "ibb"}, {"k_lamp_fast", "ibb"}, {"k_s_gen_emit", ""}};
    if (family < 0 || family >= TRC_K_FAMILIES) family = TRC_K_NONE;
    if (args) *args = names[family][1];
    return names[family][0];
}
// the instance as a kernel trace and `nm -C` spell it: "k_s_bounce<1, true, false, true, false>".  Returns the length (as snprintf).
static inline int trc_kernel_name(const trc_kernel_id &id, char *buf, size_t len) {
    const char *args;
    const char *name = trc_kernel_family_name(id.family, &args);
    int n = snprintf(buf, len, "%s%s", name, *args ? "<" : "");
    for (int k = 0; args[k]; ++k) {
        char *at = (size_t)n < len ? buf + n : nullptr;
        const size_t room = at ? len - (size_t)n : 0;
        const char *sep = args[k + 1] ? ", " : ">";
        if (args[k] == 'b') n += snprintf(at, room, "%s%s", id.a[k] ? "true" : "false", sep);
        else n += snprintf(at, room, "%d%s", id.a[k], sep);
    }
    return n;
}

static inline bool trc_src_kind_has_map(int k) {        // the source kinds a footprint map applies to (trc_fp_source)
    return k == TRC_SRC_PILLBOX_DISK || k == TRC_SRC_PILLBOX_RECT || k == TRC_SRC_BUIE_DISK || k == TRC_SRC_BUIE_RECT ||
           k == TRC_SRC_SUNSHAPE_DISK || k == TRC_SRC_SUNSHAPE_RECT;
}
static inline bool trc_src_kind_is_buie(int k) { return k == TRC_SRC_BUIE_DISK || k == TRC_SRC_BUIE_RECT; }
static inline bool trc_src_kind_is_sunshape(int k) { return k == TRC_SRC_SUNSHAPE_DISK || k == TRC_SRC_SUNSHAPE_RECT; }
static inline bool trc_src_kind_is_disc(int k) { return k == TRC_SRC_BUIE_DISK || k == TRC_SRC_PILLBOX_DISK || k == TRC_SRC_SUNSHAPE_DISK; }

// The ids the library holds an instance for: the constraints the decisions below obey, and what the id-to-pointer step of each
// family answers with a pointer.  (A family's kernels outside this set are not compiled.)
static inline bool trc_kernel_id_valid(const trc_kernel_id &id) {
    const int *a = id.a;
    const char *args;
    trc_kernel_family_name(id.family, &args);
    const int n_args = (int)strlen(args);
    for (int k = 0; k < 5; ++k)         // a bool is 0 or 1, an argument the family does not have is 0
        if (k >= n_args ? a[k] != 0 : (args[k] == 'b' && a[k] != 0 && a[k] != 1)) return false;
    switch (id.family) {
    case TRC_K_CULL: case TRC_K_FRESH: return trc_src_kind_has_map(a[0]);
    case TRC_K_UCULL: case TRC_K_FRESH2: return trc_src_kind_is_buie(a[0]);
    case TRC_K_BOUNCE:          // tables in LDS on the list of all boxes and the small grid only; fresh rays through the instance for any
                                // geometry, which alone knows the tabulated sunshapes
        return a[0] >= 0 && a[0] <= 3 && !(a[1] && a[0] >= 2) && !(a[2] && a[3]) && !(a[4] && !a[2]);
    case TRC_K_BOUNCE_COOP: return !(a[2] && !a[0]);
    case TRC_K_WALK: return a[0] == SW_THREADS;
    case TRC_K_GEN:             // continued rays; given rays; the kinds that have no k_s_gen_src
        return a[0] ? (a[1] == -1 || a[1] == TRC_SRC_BUIE_RECT || trc_src_kind_is_sunshape(a[1])) : a[1] == -1;
    case TRC_K_GEN_SRC: return a[0] == TRC_SRC_PILLBOX_DISK || a[0] == TRC_SRC_PILLBOX_RECT || a[0] == TRC_SRC_BUIE_DISK;
    case TRC_K_EXACT: case TRC_K_ABSORB: return true;
    case TRC_K_SHADE: return a[1] == 2 && !(a[4] && a[0]);          // (a chart map: the instance for any geometry and optics)
    case TRC_K_SHADE_C: return (a[0] == TRC_CLS_MIRROR || a[0] == TRC_CLS_DIFFUSE) && !(a[4] && a[1]);
    case TRC_K_SHADE_X: return !(a[3] && a[1]);                     // (no CHART x MAT instance)
    case TRC_K_TRACE_COOP: return a[0] == 512 || a[0] == 256;
    case TRC_K_TRACE_FAST: return a[0] == 256;
    case TRC_K_ORD_BOUNCE: return a[0] >= 0 && a[0] <= 2 && !(a[1] && a[2]);
    case TRC_K_SHADE_P: return true;                                // (every LDS x CHART x SPLIT)
    case TRC_K_GEN_LAMP: return trc_src_kind_is_lamp(a[0]);
    case TRC_K_LAMP_COOP: return a[0] == 512 || a[0] == 256;
    case TRC_K_LAMP_FAST: return a[0] == 256;
    case TRC_K_GEN_EMIT: return true;
    default: return false;
    }
}

// ------------------------------------------------------------------------------------------------
// DECISIONS: the streaming engine
// ------------------------------------------------------------------------------------------------
// Which candidate search the streaming engine would use for this scene -- 0 all boxes, 1 packed Kd-tree, 2 uniform grid (LDS
// sized), 3 the 32-bit grid of large scenes -- the LDS its walk kernel needs, and whether that kernel can run at all (walk_ok):
// when the tables of the search do not fit LDS the general path (k_s_gen + k_s_walk + k_s_exact) is not available and k_s_bounce
// searches for every ray from global memory.  false: no streaming form for this scene (the caller uses the megakernel).
struct StreamPlan { int mode; size_t lds_walk; bool walk_ok; };
static inline bool stream_plan(const trc_scene_facts &sc, bool want_accel, const StreamKnobs &K, StreamPlan *out) {
    if (!sc.accel_ok) return false;
    const int S = sc.n_surf;
    auto walk_lds = [&](int mode) {
        const int depth = mode == 1 ? (sc.kd_depth > 0 ? sc.kd_depth : 1) : 1;
        const size_t shared = (size_t)6 * S * 4 +
            (mode == 2 ? ((size_t)sc.grid_cells + 1 + 2 + (size_t)sc.grid_list) * 2
                       : (mode == 1 ? ((size_t)2 * sc.kd_nodes * 4 + (size_t)sc.kd_nleaf * 2) : (8 + (size_t)sc.brute_list * 2))) + 32;
        return shared + (size_t)(SW_THREADS / 64) * SW_WAVE_BYTES(depth);
    };
    int mode = 0;
    if (want_accel) {
        // the uniform grid of trc_bounds.h; TRC_STREAM_SEARCH=1 walks the caller's Kd-tree instead (when its walk kernel fits)
        const bool kd_fits = sc.accel_kd_ok && S <= TRC_MAX_SURFACES16 && walk_lds(1) <= LDS_MAX_ALLOWED;
        if (K.search == 1 && kd_fits) mode = 1;
        else if (sc.grid_ok) mode = 2;
        else if (sc.big_ok) mode = 3;       // a scene beyond the LDS-sized structures: the 32-bit grid in global memory
        else if (kd_fits) mode = 1;
    }
    if (mode == 0 && S > TRC_MAX_SURFACES16) return false;      // (the list of all boxes holds 16-bit numbers)
    size_t lds = mode == 3 ? 0 : walk_lds(mode);
    const bool walk_ok = mode != 3 && lds <= LDS_MAX_ALLOWED;
    if (!walk_ok) lds = 0;
    out->mode = mode;
    out->lds_walk = lds;
    out->walk_ok = walk_ok;
    return true;
}

// one kernel instance of a stage: its id (family TRC_K_NONE: the call has no such stage), threads per workgroup, dynamic LDS
struct trc_stage { trc_kernel_id id; int threads; size_t lds; };
// ... of a shading kernel: the class it serves (-1: the only shading kernel, every kind) and the tables it stages
struct trc_shade_stage { trc_kernel_id id; int threads; size_t lds; int cls, lds_tables, lds_fm_bins; };

// k_s_shade_p's image: that of TRC_IMG_SHADE_X with the sample grid and the birth vector (W doubles each) behind it.  They belong to
// the tables -- all in LDS or none, so that every access has a known address space: the LDS instance serves a call whose image fits
// the kernel's limit WITH them, and a long optics table or a long grid sends the tables, the grid and the birth vector to global
// memory together.  The lambda cells of the polychromatic walls (per wall and sample a weight and a cell, and a word per surface)
// follow when they fit the same limit too: *cells = the walls staged, all of them or 0 (then every hit searches).
static inline size_t trc_poly_grid_bytes(int W) { return (size_t)16 * (size_t)W; }
static inline size_t trc_poly_cells_bytes(int W, int walls, int n_surf) {
    return (size_t)walls * W * 8 + (((size_t)walls * W + 1) / 2) * 8 + (((size_t)n_surf + 1) / 2) * 8;
}
static inline size_t trc_shade_p_choose(const trc_scene_facts &sc, int W, int walls, bool *in_lds, int *lds_fm_bins, int *cells) {
    const int img = TRC_IMG_SHADE_X;
    auto need = [&](bool lds, int bins) {
        const trc_shade_layout L = trc_shade_lds_layout(trc_shade_lds_parts(img, lds, sc.n_surf, sc.stride, sc.n_fm_edges, sc.fms_bytes, sc.n_extra, bins));
        return L.end + L.slack + (lds ? trc_poly_grid_bytes(W) : 0);
    };
    *in_lds = need(true, 0) <= trc_shade_lds_limit(img, false);
    *lds_fm_bins = (sc.fm_bins > 0 && *in_lds && need(true, (int)sc.fm_bins) <= trc_shade_lds_limit(img, true)) ? (int)sc.fm_bins : 0;
    size_t lds = need(*in_lds, *lds_fm_bins);
    const size_t b_cells = trc_poly_cells_bytes(W, walls, sc.n_surf);
    *cells = (*in_lds && walls > 0 && lds + b_cells <= trc_shade_lds_limit(img, *lds_fm_bins > 0)) ? walls : 0;
    if (*cells) lds += b_cells;
    return lds;
}

// The kernels a streaming call runs and the per-call decisions its bounces are planned by
struct trc_stream_forms {
    int src_kind;
    int gridm;                   // k_s_bounce's form of the search: 0 all boxes, 1 LDS-sized grid, 2 large grid, 3 surface by surface
    bool small_scene;
    trc_stage gen0, gen, walk, exact;       // the general path: k_s_gen for fresh / for continued rays, k_s_walk, k_s_exact
    trc_shade_stage shk[TRC_CLS_COUNT];
    int n_shk;
    bool multi;                  // more than one shading kernel: k_s_partition parts the hit list by class first
    trc_stage cull, fresh, fresh_one;       // fresh_one: k_s_fresh itself where `fresh` is its two-phase form
    trc_stage cull_u;            // k_s_ucull on the mask over the uniforms, in front of k_s_fresh2
    int cull_lu, cull_lv;        // ... whose dimensions are 1 << lu, 1 << lv
    double ulisted_share;        // ... and the share of the fresh rays it lists
    trc_stage bounce, first, absorb;        // k_s_bounce for continued rays / for fresh ones, k_s_absorb
    bool coop;                   // k_s_bounce_coop serves the large grid (it lists terminal hits, never finishes them itself)
    bool use_fp, use_fused, use_first, use_absorb, absorb_inline;
    size_t lds_inline;           // absorb_inline: the bytes of bounce.lds that hold k_s_absorb's tables (the grid cap is set without them)
    double general_share;       // expected share of the fresh rays that k_s_cull leaves to the general path
    double listed_share;         // ... and lists for k_s_fresh (an estimate for its grid: the covered part of the source)
    // what the choice sets in StreamParams
    int search, lds_recs, lds_tally, lds_tables, lds_extra, lds_fm_bins, bg_occ_words, shade_term_cls, split_terminal;
    int poly_cells;              // CarryIn.poly_cells: the polychromatic walls whose lambda cells k_s_shade_p stages (0 for every other call)
    bool ahead;                  // StreamParams.ahead: k_s_shade_c finishes the next segment of the rays inside their clear cones (trc_stream_form_ahead)
};

static inline trc_lds_parts trc_fresh_parts(const trc_facts &f, bool buie, bool lds, int queue_waves) {
    trc_fp_params P = {};
    P.Mc = f.fp.Mc;
    return fresh_lds_parts(f.scene.n_surf, f.scene.stride, P, f.fp.n_list, buie, lds, queue_waves);
}

// the general path: k_s_gen, k_s_walk (the tables of the search in LDS), k_s_exact (the records in LDS when they fit)
static inline void trc_stream_form_general(trc_stream_forms &F, const trc_facts &f, const StreamPlan &plan) {
    const size_t b_recs = (size_t)f.scene.n_surf * f.scene.stride * 8;
    const size_t lds_exact = b_recs <= TRC_EXACT_RECS_LIMIT ? b_recs : 0;
    F.lds_recs = lds_exact ? 1 : 0;
    const int k = F.src_kind;
    // fresh rays: the kinds with a generation kernel of their own, the others through k_s_gen<true, KIND>, given rays through <true, -1>
    // (the lamp kinds have no source plane, hence no footprint map: every fresh ray of theirs comes this way, through k_s_gen_lamp<KIND>)
    // (the thermal emitters likewise, through k_s_gen_emit)
    const trc_kernel_id gen0 = trc_src_kind_is_lamp(k) ? trc_kid(TRC_K_GEN_LAMP, k)
                             : k == TRC_SRC_EMIT_THERMAL ? trc_kid(TRC_K_GEN_EMIT)
                             : (k == TRC_SRC_BUIE_DISK || k == TRC_SRC_PILLBOX_DISK || k == TRC_SRC_PILLBOX_RECT) ? trc_kid(TRC_K_GEN_SRC, k)
                             : trc_kid(TRC_K_GEN, 1, (k == TRC_SRC_BUIE_RECT || trc_src_kind_is_sunshape(k)) ? k : -1);
    F.gen0 = {gen0, 256, 0};
    F.gen = {trc_kid(TRC_K_GEN, 0, -1), 256, 0};
    // (the general path never runs on tables beyond LDS: there `search` == plan.mode)
    F.walk = {trc_kid(TRC_K_WALK, SW_THREADS, plan.mode == 2), SW_THREADS, plan.lds_walk};
    F.exact = {trc_kid(TRC_K_EXACT), 256, lds_exact};
}

// The shading kernels: one per optics class present in the scene (trc_shade.hip), each taking its hits off the bounce's list, or one
// for every hit (k_s_shade_x) when the rays carry more than the fast engine's record (carry), among them the calls on a scene whose
// optics send two rays on from a hit (its SPLIT form) -- k_s_shade_p in its place when the source carries its spectrum (poly_src).
// false: no instance (device material tables beside a chart flux map, or beside a carried spectrum).
static inline bool trc_stream_form_shade(trc_stream_forms &F, const trc_facts &f) {
    const trc_scene_facts &sc = f.scene;
    const bool carry = f.call.carry, spec = f.call.spec, chart = sc.chart;
    auto choose = [&](int img, bool *in_lds, int *bins_in) {
        return trc_shade_lds_choose(img, sc.n_surf, sc.stride, sc.n_fm_edges, sc.fms_bytes, sc.n_extra, sc.fm_bins, in_lds, bins_in);
    };
    // k_s_shade, or k_s_shade_x for rays that carry more (the same image): tallies, records, optics parameters, flux-map tables, flags
    // and table values in LDS -- all of them or none (its LDS instance knows the address space of every table; see the kernel) -- and
    // the flux-map bins too while a workgroup stays within half a CU's LDS (two workgroups per CU)
    // (k_s_shade_p, for a source that carries its spectrum: the same image with grid, birth vector and cells, trc_shade_p_choose)
    const bool poly = carry && f.call.poly_src > 0;
    bool shade_lds;
    F.poly_cells = 0;
    const size_t lds_shade = poly ? trc_shade_p_choose(sc, f.call.poly_src, f.call.poly_walls, &shade_lds, &F.lds_fm_bins, &F.poly_cells)
                                  : choose(carry ? TRC_IMG_SHADE_X : TRC_IMG_SHADE, &shade_lds, &F.lds_fm_bins);
    F.lds_tally = F.lds_tables = F.lds_extra = shade_lds ? 1 : 0;
    // A flux map in another chart than XY: the instances that know the charts -- of k_s_shade and of the lean kernels the ones for
    // any geometry and any optics, which serve flat mirrors and walls with the same arithmetic.  Hits on surfaces that end every ray
    // go to the shading kernels in such a scene (trc_stream_form_absorb): k_s_absorb and k_s_bounce have no such instance.
    // (k_s_shade: instances built for 3 and 4 waves per SIMD -- 168 / 128 registers, 228 / 376 bytes of scratch per lane -- were slower:
    // 3.09 and 2.70 ms per NSTTF step against 2.54; later, without anything fetched ahead and with the incidence-angle factor out
    // of line, 192 / 336 bytes and 2.33 / 2.35 ms against 1.99.  The registers are held by the optics code as a whole -- an instance
    // that only knows Transparent needs none of the spills -- and it does not yield to the obvious: lighter sine / cosine / tangent
    // kernels for bounded arguments made it worse (their float64 constants live in scalar registers, which then spill into vector
    // ones))
    int n_shk = 0, term_cls = -1;
    unsigned present = 0u;
    if (!carry) {
        // a surface that ends every ray (TRC_SURF_TERMINAL) needs no optics when a ray of energy 0 ends in the reference too
        // (0 <= min_energy): its hits go to a class that is there anyway
        const bool any_term = f.call.term_ok && sc.any_term;
        present = f.call.term_ok ? sc.cls_moving : sc.cls_all;
        if (any_term) {
            term_cls = (present >> TRC_CLS_MIRROR) & 1u ? TRC_CLS_MIRROR : (present >> TRC_CLS_DIFFUSE) & 1u ? TRC_CLS_DIFFUSE : -1;
            if (term_cls < 0) present = sc.cls_all;       // nothing lean among the others: the terminal surfaces go by their own class
        }
        const bool all_flat = !chart && sc.all_flat;
        for (int c = 0; c < TRC_CLS_GENERAL; ++c) {
            if (!((present >> c) & 1u)) continue;
            trc_shade_stage &K = F.shk[n_shk++];
            bool in_lds;
            K.cls = c; K.threads = SHC_THREADS;
            K.lds = choose(c == TRC_CLS_MIRROR ? TRC_IMG_LEAN_MIRROR : TRC_IMG_LEAN, &in_lds, &K.lds_fm_bins);
            K.lds_tables = in_lds ? 1 : 0;
            K.id = trc_kid(TRC_K_SHADE_C, c, all_flat, in_lds, spec, chart);
        }
    }
    if (carry || ((present >> TRC_CLS_GENERAL) & 1u)) {
        trc_shade_stage &K = F.shk[n_shk++];
        K.cls = carry ? -1 : TRC_CLS_GENERAL;
        K.lds = lds_shade; K.lds_tables = F.lds_tables; K.lds_fm_bins = F.lds_fm_bins;
        if (carry) {            // sixteen waves per workgroup; the MAT instances read the materials' tables on the device
            if (f.call.mat_dev && (chart || poly)) return false;       // (nor a MAT instance of k_s_shade_p)
            K.id = poly ? trc_kid(TRC_K_SHADE_P, shade_lds, chart, sc.splits) : trc_kid(TRC_K_SHADE_X, shade_lds, chart, sc.splits, f.call.mat_dev);
            K.threads = SHC_THREADS;
        } else {                // 2 waves per SIMD: four workgroups of 256 per CU in two rounds; scenes of flat surfaces with mirror /
                                // diffuse optics only (heliostat fields, plate cavities): the SIMPLE instance
            K.id = trc_kid(TRC_K_SHADE, sc.simple && !chart, 2, shade_lds, spec, chart);
            K.threads = SH_THREADS;
        }
    }
    F.n_shk = n_shk;
    F.multi = n_shk > 1;
    F.shade_term_cls = term_cls;
    return true;
}

// fresh rays of a plane source with a narrow cone: footprint map, k_s_cull + k_s_fresh (trc_footprint.h)
static inline void trc_stream_form_fresh(trc_stream_forms &F, const trc_facts &f) {
    F.general_share = 0.0; F.listed_share = 1.0;
    F.use_fp = f.fp.use;
    if (!F.use_fp) return;
    const int kind = F.src_kind;
    const bool buie = trc_src_kind_is_buie(kind), flat = f.scene.all_flat;
    const int sf_threads = SF_THREADS(flat);
    // the Buie sources go through the two-phase form (k_s_fresh2): a queue of SFQ_CAP (ray, cell) pairs per wave
    const bool fresh_two = buie;
    const int queue_waves = fresh_two ? sf_threads / 64 : 0;
    // k_s_fresh: the tables every listed ray reads go to LDS when they all fit (one workgroup per CU); the lists are 16-bit there
    const bool in_lds = f.fp.n_list < TRC_FP_LIST_LIMIT && lds_need(trc_search_lds_layout(trc_fresh_parts(f, buie, true, queue_waves))) <= TRC_SEARCH_LDS_LIMIT;
    const size_t lds_fresh = lds_request(trc_search_lds_layout(trc_fresh_parts(f, buie, in_lds, queue_waves)));
    const size_t lds_cull = (size_t)f.fp.M * f.fp.M / 8 + (SC_GEN_CAP + 4) * 4;
    if (lds_cull > LDS_MAX_ALLOWED || lds_fresh > LDS_MAX_ALLOWED) { F.use_fp = false; return; }
    // (the tabulated sunshapes: the general <kind, flat, lds> form, their table read from global memory, where it stays in L2)
    F.fresh_one = {trc_kid(TRC_K_FRESH, kind, flat, in_lds), sf_threads, lds_fresh};
    F.fresh = fresh_two ? trc_stage{trc_kid(TRC_K_FRESH2, kind, flat, in_lds), sf_threads, lds_fresh} : F.fresh_one;
    F.cull = {trc_kid(TRC_K_CULL, kind), SC_THREADS, lds_cull};
    F.ulisted_share = 1.0;
    // The mask over the uniforms, for the listed rays that k_s_fresh2 takes: it finds its list cell itself.  k_s_fresh (the
    // pillbox kinds, the tabulated sunshapes, a Buie source whose listed rays mostly hit) and the instances of k_s_fresh2 that
    // do not derive the cell (SF2_DERIVES_CELL) are handed it by the other form.
    if (fresh_two && SF2_DERIVES_CELL(flat, in_lds) && f.knobs.umask && f.fp.umask_words > 0) {
        F.cull_u = {trc_kid(TRC_K_UCULL, kind), SC_THREADS, (size_t)f.fp.umask_words * 4 + (SC_GEN_CAP + 4) * 4};      // (at most what the Cartesian mask takes: Mu Mv <= M M)
        for (F.cull_lu = 0; (1 << F.cull_lu) < f.fp.Mu; ++F.cull_lu) {}
        for (F.cull_lv = 0; (1 << F.cull_lv) < f.fp.Mv; ++F.cull_lv) {}
        F.ulisted_share = f.fp.ucoverage > 1.0 ? 1.0 : f.fp.ucoverage;
    }
    F.general_share = f.fp.has_generic ? (1.0 - f.fp.cdf_end) : 0.0;
    if (F.general_share < 0.0) F.general_share = 0.0;
    F.listed_share = f.fp.coverage * (trc_src_kind_is_disc(kind) ? 4.0 / TRC_PI : 1.0);      // (the mask is a square around the disc)
    if (F.listed_share > 1.0) F.listed_share = 1.0;
}

// Continued rays (bounces >= 1): one kernel per bounce on the grid / all-boxes forms (k_s_bounce); the Kd walk of
// TRC_STREAM_SEARCH=1 keeps the queues.  Fresh rays outside the footprint map go through k_s_bounce<.., FRESH> instead of the
// general path in large scenes and in small ones.
static inline void trc_stream_form_bounce(trc_stream_forms &F, const trc_facts &f, const StreamPlan &plan) {
    const trc_scene_facts &sc = f.scene;
    const int S = sc.n_surf;
    const bool big = !plan.walk_ok;
    F.use_fused = plan.mode != 1 && (f.knobs.bounce || big);
    // (k_s_bounce<.., FRESH> does not know the lamp kinds: their fresh rays take the general path, and trc_fast_choose_engine gives a
    // scene without one to the megakernel)
    F.use_first = !trc_src_kind_is_emitter(F.src_kind) && (big || F.small_scene || (f.knobs.first && plan.mode != 1));
    if (!F.use_fused && !F.use_first) return;
    const int gridm = F.gridm;
    // One decision for the instance of the continued rays and that of the fresh ones: the tables go to LDS when an image with the
    // parts of both (the Buie table of the one, the flags of the other) fits; the fresh instance is sized by that image
    const int g_cells = plan.mode == 2 ? sc.grid_cells : 0, g_list = sc.grid_list;
    const bool in_lds = gridm != 2 && gridm != 3 && lds_need(trc_search_lds_layout(bounce_lds_parts(S, sc.stride, true, true, true, g_cells, g_list, 0, 0))) <= TRC_SEARCH_LDS_LIMIT;
    // the large grid: k_s_bounce_coop, whose lanes share the tests of their wave's rays
    const bool coop = F.coop = gridm == 2 && f.knobs.coop;
    if (gridm == 2 && (size_t)sc.big_occ_words * 4 <= (size_t)(coop ? TRC_BG_OCC_COOP_BYTES : TRC_BG_OCC_LANES_BYTES)) F.bg_occ_words = sc.big_occ_words;      // the occupancy bits of the large grid
    const int coop_waves = coop ? SB_THREADS / 64 : 0;
    auto request = [&](bool fresh) {
        return lds_request(trc_search_lds_layout(bounce_lds_parts(S, sc.stride, fresh, in_lds, in_lds, in_lds ? g_cells : 0, g_list, F.bg_occ_words, coop_waves)));
    };
    // (fresh rays: the instance for any geometry -- k_s_bounce_coop has a flat one too -- which alone knows the tabulated sunshapes)
    const bool all_flat = sc.all_flat, sun = trc_src_kind_is_sunshape(F.src_kind);
    F.bounce = {coop ? trc_kid(TRC_K_BOUNCE_COOP, 0, all_flat, 0) : trc_kid(TRC_K_BOUNCE, gridm, in_lds, 0, all_flat, 0), SB_THREADS_OF(gridm), request(false)};
    F.first = {coop ? trc_kid(TRC_K_BOUNCE_COOP, 1, all_flat, sun) : trc_kid(TRC_K_BOUNCE, gridm, in_lds, 1, 0, sun), SB_THREADS_OF(gridm), request(true)};
}

// Hits on surfaces that end every ray (the receiver of a field) are listed apart by k_s_bounce and finished by k_s_absorb -- when
// the scene has such surfaces and k_s_absorb's tables (those of k_s_shade without records and optics) fit LDS -- or finished inside
// k_s_bounce when its workgroup has the LDS for the tallies, flux-map tables and bins as well (TRC_STREAM_ABSORB=1: always behind
// the list, by k_s_absorb).
static inline void trc_stream_form_absorb(trc_stream_forms &F, const trc_facts &f) {
    const trc_scene_facts &sc = f.scene;
    if (!(F.use_fused && F.lds_tally && F.lds_tables && !f.call.carry)) return;
    auto need = [&](int img) { return shade_lds_need(trc_shade_lds_parts(img, true, sc.n_surf, sc.stride, sc.n_fm_edges, sc.fms_bytes, sc.n_extra, F.lds_fm_bins)); };
    const size_t lds_absorb = need(TRC_IMG_ABSORB);
    const bool fm_ok = sc.fm_bins == 0 || F.lds_fm_bins > 0;   // (bins outside LDS would be scattered global atomics at eight waves per SIMD: not this kernel;
                                                                // nor a map in another chart than XY: k_s_absorb and k_s_bounce bin in x, y only)
    F.use_absorb = sc.any_term && fm_ok && !sc.chart && lds_absorb <= trc_shade_lds_limit(TRC_IMG_ABSORB, true) && !sc.transfer && f.call.term_ok && f.knobs.absorb != 0;      // (0 <= min_energy: the ray ends there in the reference too)
    if (!F.use_absorb) return;
    // one workgroup of 16 waves per CU (4096 waves with open chunks of the hit buffer at most)
    F.absorb = {trc_kid(TRC_K_ABSORB), SA_THREADS, lds_absorb};
    F.split_terminal = 1;
    const size_t extra_lds = need(TRC_IMG_INLINE);
    if (f.knobs.absorb != 1 && !(F.gridm == 2 && F.coop) && F.bounce.lds + extra_lds <= trc_shade_lds_limit(TRC_IMG_INLINE, true)) {
        F.absorb_inline = true;
        F.lds_inline = extra_lds;
        F.bounce.lds += extra_lds;
        F.split_terminal = 2;
    }
}

// The shading instances that can finish a continued ray's next segment themselves (k_s_shade_c's AHEAD, trc_shade.hip): the mirror
// class with flat normals and its tables in LDS, without a spectrum to draw and without flux-map charts
static inline bool trc_shade_finishes_ahead(const trc_kernel_id &id) {
    return id.family == TRC_K_SHADE_C && id.a[0] == TRC_CLS_MIRROR && id.a[1] == 1 && id.a[2] == 1 && id.a[3] == 0 && id.a[4] == 0;
}

// A mirror's ray inside the clear cone of the tile it leaves does not walk the grid in k_s_bounce<1, .., FRESH = false>: that kernel
// tests the surfaces set apart for it and, with split_terminal == 2, finishes a hit on one that ends every ray in place.  The
// shading kernel that reflects the ray does the same while it has the ray in registers, and the ray's record, its energy and its
// entry of the active list are never written (k_s_shade_c, AHEAD).  On for a call when the next bounce's search is that kernel with
// the clear cones and finishes terminal hits itself, no surface is without a box (those k_s_bounce tests for every ray), and an
// instance that knows the path shades; TRC_STREAM_AHEAD=0 leaves every continued ray to k_s_bounce.
static inline void trc_stream_form_ahead(trc_stream_forms &F, const trc_facts &f) {
    F.ahead = false;
    if (!(F.use_fused && F.gridm == 1 && F.bounce.id.family == TRC_K_BOUNCE && F.bounce.id.a[0] == 1 && F.bounce.id.a[2] == 0)) return;
    if (F.split_terminal != 2 || !f.scene.clear_cones || !f.knobs.clear || f.scene.n_unbounded != 0 || !f.knobs.ahead) return;
    for (int k = 0; k < F.n_shk; ++k) F.ahead = F.ahead || trc_shade_finishes_ahead(F.shk[k].id);
}

// Chooses the kernel of every stage of a streaming call (f.scene walked, f.fp as stream_fp_prepare left it, f.call.carry with the
// calls on a scene whose optics split rays).  false: no shading kernel for this call (trc_stream_form_shade).
static inline bool trc_stream_decide(const trc_facts &f, const StreamPlan &plan, trc_stream_forms *out) {
    trc_stream_forms &F = *out;
    memset(&F, 0, sizeof(F));
    const int S = f.scene.n_surf;
    F.src_kind = f.call.src_kind;
    F.gridm = plan.mode == 2 ? 1 : (plan.mode == 3 ? 2 : 0);
    // a few surfaces: neither grid nor lists, the wave takes the surfaces one by one (k_s_bounce<3>) -- up to four surfaces (a
    // dish and its receiver), where every lane tests every surface anyway and the form pays: 0.50 against 0.58 ms per bounce of
    // 1e7 rays.  (Measured on the seven-wall cavity, one batch alone: 1.15 ms per bounce surface by surface against 0.96 ms lane by
    // lane -- every wave runs all seven exact tests where its lanes needed four or five each.)
    F.small_scene = S <= STREAM_SMALL_SURFACES && plan.mode != 1 && plan.walk_ok;
    if (F.small_scene && S <= STREAM_TINY_SURFACES) F.gridm = 3;
    F.search = plan.walk_ok ? plan.mode : 2;
    trc_stream_form_general(F, f, plan);
    if (!trc_stream_form_shade(F, f)) return false;
    trc_stream_form_fresh(F, f);
    trc_stream_form_bounce(F, f, plan);
    trc_stream_form_absorb(F, f);
    trc_stream_form_ahead(F, f);
    return true;
}

// ------------------------------------------------------------------------------------------------
// DECISIONS: the megakernel, the engine of a fast call, the ordered engine
// ------------------------------------------------------------------------------------------------
// The megakernel's LDS budget.  Preferred (m32): k_trace_coop, the single-precision conservative search with everything it needs
// in LDS, 512 threads or 256; else k_trace_fast with the tallies and the scene in LDS as far as they fit.  Its instance: for a source
// with a spectrum (SPEC: it draws the wavelength), a tabulated sunshape (SUN) and a scene with a flux map in another chart than XY
// (CHART).
struct MegaPlan {
    bool m32;
    int threads;
    size_t lds;
    int lds_tally, lds_scene;
    trc_kernel_id id;
};
static inline MegaPlan mega_plan(const trc_scene_facts &sc, const trc_call_facts &c) {
    const int S = sc.n_surf;
    const bool accel = sc.has_kd && (c.flags & TRC_TRACE_ACCEL);       // (without a Kd-tree the megakernel tests every box)
    const size_t b_buie = c.src_kind >= 0 ? (size_t)TRC_BUIE_STAGED * 8 : 0;
    const size_t b_tally = (size_t)(3 * S + 2) * 8;
    MegaPlan M = {false, 256, 0, 0, 0, {}};
    if (sc.accel_ok && S <= TRC_MAX_SURFACES16 && (!accel || (sc.accel_kd_ok && sc.kd_nodes <= COOP_MAX_NODES && sc.kd_depth <= COOP_MAX_DEPTH))) {
        const size_t b_acc = (size_t)6 * S * 4 + (accel ? ((size_t)2 * sc.kd_nodes * 4 + (size_t)sc.kd_nalways * 4 + (size_t)sc.kd_nleaf * 2)
                                                        : (8 + (size_t)sc.brute_list * 2)) +
                             (size_t)sc.n_unbounded * 4 + 32;
        const size_t b_wave = COOP_WAVE_BYTES(accel ? (sc.kd_depth > 0 ? sc.kd_depth : 1) : 1);
        for (int threads = 512; threads >= 256 && !M.m32; threads /= 2) {
            const size_t lds = b_buie + b_tally + b_acc + (size_t)(threads / 64) * b_wave;
            if (lds <= LDS_MAX_ALLOWED) M = {true, threads, lds, 1, 0, {}};
        }
    }
    if (!M.m32) {
        size_t b_scene = (size_t)S * sc.stride * 8;
        if (sc.has_kd) b_scene += (size_t)sc.kd_nodes * 8 + ((size_t)sc.kd_nodes * 2 + sc.kd_nleaf + sc.kd_nalways) * 4 + 8;
        M.lds = b_buie;
        M.lds_tally = (M.lds + b_tally <= LDS_MAX_PLAIN) ? 1 : 0;
        if (M.lds_tally) M.lds += b_tally;
        M.lds_scene = (M.lds + b_scene <= LDS_MAX_PLAIN) ? 1 : 0;
        if (M.lds_scene) M.lds += b_scene;
    }
    if (trc_src_kind_is_emitter(c.src_kind)) M.id = trc_kid(M.m32 ? TRC_K_LAMP_COOP : TRC_K_LAMP_FAST, M.threads, c.spec, sc.chart);
    else M.id = trc_kid(M.m32 ? TRC_K_TRACE_COOP : TRC_K_TRACE_FAST, M.threads, c.spec, trc_src_kind_is_sunshape(c.src_kind), sc.chart);
    return M;
}

// Large calls run the streaming engine (phases as separate kernels connected by HBM queues, trc_stream.inc); small ones the
// persistent megakernel, which needs one launch and no workspace.  TRC_TRACE_STREAM / TRC_TRACE_MEGAKERNEL force one or the other.
// refused: the call's rays or the scene's optics are the streaming form's alone, and the scene has none.
struct trc_engine_choice { StreamPlan plan; bool use_stream, refused; };
static inline trc_engine_choice trc_fast_choose_engine(const trc_scene_facts &sc, const trc_call_facts &c, const StreamKnobs &K) {
    trc_engine_choice E = {{0, 0, true}, false, false};
    bool stream_ok = c.n >= TRC_STREAM_FEWEST_RAYS && stream_plan(sc, (c.flags & TRC_TRACE_ACCEL) != 0, K, &E.plan);
    // (a lamp's fresh rays need the general path, which a scene whose search tables do not fit LDS has not)
    if (trc_src_kind_is_emitter(c.src_kind) && !E.plan.walk_ok) stream_ok = false;
    // (rays that carry more, and optics that send two rays on from a hit, are the streaming form's alone: k_s_shade_x)
    const bool stream_only = c.carry || sc.splits;
    const bool force_stream = (c.flags & TRC_TRACE_STREAM) || stream_only;
    const bool force_mega = !stream_only && (c.flags & TRC_TRACE_MEGAKERNEL);
    // (a scene on the large grid -- a mesh of 1e5 faces -- has nothing but its boxes to search in the megakernel: 2e5 rays on the
    // relief of 105 800 triangles took 570 ms there, 1.3 ms here)
    const long long stream_from = E.plan.mode == 3 ? TRC_STREAM_MIN_RAYS_BIG : TRC_STREAM_MIN_RAYS;
    E.use_stream = stream_ok && (force_stream || (!force_mega && c.n >= stream_from));
    E.refused = stream_only && !E.use_stream;
    return E;
}

// the search of k_ord_bounce: 2 the large grid (the scene stands on it and the caller brought no tree), 1 the single-precision
// conservative search, 0 the generic one; its instance knows the flux-map charts (CHART), or the materials' tables on the device (MAT)
struct trc_ord_choice { int mode; trc_kernel_id id; };
static inline trc_ord_choice trc_ordered_choose(const trc_scene_facts &sc, int flags, bool mat_dev) {
    const bool use_kd = sc.has_kd && (flags & TRC_TRACE_ACCEL);
    int mode = 0;
    if (sc.accel_ok && sc.big_ok && !use_kd) mode = 2;
    else if (sc.accel_ok && sc.n_surf <= TRC_MAX_SURFACES16 && (!use_kd || (sc.accel_kd_ok && sc.kd_depth + 2 <= ORD_STACK_DEPTH))) mode = 1;
    return {mode, trc_kid(TRC_K_ORD_BOUNCE, mode, sc.chart, !sc.chart && mat_dev)};
}

#endif
