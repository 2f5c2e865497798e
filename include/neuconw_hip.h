/* neuconw_hip.h -- C ABI of libneuconw_hip.so: the MI355X (gfx950) native hot path of
 * NeuralRecon-W's volume renderer.
 *
 * The reference (zju3dv/NeuralRecon-W) has no FFI: its hot path is Python calling torch ops.  The
 * entry points below are the functions a maintainer would bind (ctypes -- see INTEGRATION.md) to
 * replace, one for one, the torch-op bodies of
 *     rendering/renderer.py  (sample_pdf :15-48, up_sample :257-341, cat_z_vals :343-363,
 *                             render_core_outside :157-228, render_core :570-783,
 *                             get_near_far_* :380-456)
 *     models/neuconw.py      (SDFNetwork :183-296, RenderingNetwork :59-170, NeuconW :299-376)
 *     models/nerf.py         (NeRF :86-183)
 *     tools/prepare_data/generate_voxel.py  (get_near_far :311-439, kaolin raytrace)
 *
 * Conventions: all pointers are DEVICE pointers unless a parameter is documented as a host
 * struct; `stream` is a hipStream_t passed as void*; every function is asynchronous on `stream`
 * and returns 0 on success or a hipError_t / negative NCW_E_* code.  No torch types appear here.
 * prec: 0 = exact-fp32 MFMA (v_mfma_f32_32x32x2_f32; parity mode), 1 = bf16 MFMA with f32
 * accumulation (v_mfma_f32_32x32x16_bf16; throughput mode), 2 = fp16 MFMA with f32 accumulation
 * (v_mfma_f32_32x32x16_f16: the same kernels compiled a second time with the 16-bit type switched -- 8x the mantissa
 * of bf16 at the same speed; the library also exports every MLP entry point as <name>_f16, which is what prec 2
 * dispatches to).  Packed weights and stashes of a network must be built with the prec they are used with.
 */
#ifndef NEUCONW_HIP_H
#define NEUCONW_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCW_PREC_F32 0
#define NCW_PREC_BF16 1
#define NCW_PREC_F16 2   /* fp16 operands (10 mantissa bits), f32 accumulate; the caller loss-scales the backward */
#define NCW_MAX_LAYERS 12
#define NCW_MAX_SEGS 4

#define NCW_E_BADARG (-1)
#define NCW_E_UNSUPPORTED (-2)

/* library / device info; returns the ABI version (bumped on any signature change) */
int ncw_abi_version(void);
/* sha256 (hex) of the sources this library was built from (every .hip / .h file of csrc/ and this header); the Python binding
 * refuses a library whose hash differs from the tree's (neuralrecon-w_amd/build.py source_hash) */
const char* ncw_source_hash(void);
/* writes "gfx950" style arch name of device 0 into buf; returns CU count (0 if no device) */
int ncw_device_info(char* buf, int buflen);

/* ------------------------------------------------------------------------------------------
 * Weight packing (replaces nn.utils.weight_norm's reparametrisation + the implicit cuBLAS
 * operand layout; models/neuconw.py:104-105,256-257).  One descriptor = one nn.Linear (or a row
 * range of it) scattered into one zero-padded matrix in MFMA fragment order.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwSeg {
    int32_t col0;   /* first source column of the segment                       */
    int32_t ncols;  /* number of source columns                                 */
    int32_t dcol0;  /* destination (padded, logical) input-feature index        */
    int32_t _pad;
} NcwSeg;

typedef struct NcwPackDesc {
    const float* src;    /* weight (or weight_v) [rows_total, ld] row-major     */
    const float* g;      /* weight_g [rows_total] or NULL (plain Linear)        */
    const float* bias;   /* bias [rows_total] or NULL                            */
    void* dst_w;         /* packed matrix (pre-zeroed once; padding never rewritten) */
    float* dst_b;        /* packed bias [rb_out*32] (C-layout order) or NULL    */
    int32_t ld;          /* source leading dimension = in_features               */
    int32_t row0, nrows; /* source row range packed by this descriptor           */
    int32_t drow0;       /* destination (padded, logical) output-feature index   */
    int32_t rb_out, rb_in; /* destination block dims (x32) in its own orientation */
    int32_t transpose;   /* 1: destination is the transpose (out<->in swapped)    */
    int32_t prec;        /* element type of dst_w                                 */
    float scale;         /* e.g. 1/sqrt(2) folded into the skip layer             */
    int32_t nseg;
    NcwSeg seg[NCW_MAX_SEGS];
    int32_t residual;    /* 16-bit only: 1 = store the ROUNDING RESIDUAL lo = h16(w - h16(w)) instead of h16(w): the
                          * second half of a split (hi + lo) weight matrix, NcwSdfNet.w_lo */
    int32_t _pad;
} NcwPackDesc;

/* descs: device array of n descriptors; row_prefix: device int32[n+1] exclusive prefix sum of
 * nrows (grid = row_prefix[n] blocks, passed as total_rows). */
int ncw_pack_weights(const NcwPackDesc* descs, const int32_t* row_prefix, int n, int total_rows,
                     void* stream);

/* Reverse of ncw_pack_weights for gradients: reads the dense padded gradient matrices produced by
 * ncw_wgrad and writes d(weight_g), d(weight_v) / d(weight), d(bias) of the original parameters
 * (weight-norm backward: g_bar = sum(Wbar * v/|v|), v_bar = g/|v| (Wbar - g_bar v/|v|)). */
typedef struct NcwUnpackDesc {
    const float* dw;     /* dense padded gradient [rb_out*32, ldw], forward orientation */
    const float* db;     /* dense padded bias gradient [rb_out*32] or NULL               */
    const float* src;    /* weight_v / weight                                            */
    const float* g;      /* weight_g or NULL                                             */
    float* d_src;        /* out: grad of weight_v / weight  [rows_total, ld]             */
    float* d_g;          /* out: grad of weight_g or NULL                                */
    float* d_bias;       /* out: grad of bias or NULL                                    */
    int32_t ld, ldw;
    int32_t row0, nrows, drow0;
    float scale;
    float grad_mul;      /* multiplies every gradient written (0 = 1): 1 / loss scale in the fp16 mode */
    int32_t accumulate;  /* 1: add into d_* (torch .grad accumulation), 0: overwrite     */
    int32_t nseg;
    NcwSeg seg[NCW_MAX_SEGS];
    const float* grad_mul_dev; /* device scalar multiplied on top of grad_mul (the dynamic 1 / loss scale) or NULL */
} NcwUnpackDesc;
int ncw_unpack_grads(const NcwUnpackDesc* descs, const int32_t* row_prefix, int n, int total_rows,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * SDF network (models/neuconw.py:183-296).  HOST struct of device pointers to packed weights.
 * Layer l in [0, n_layers): w[l] = packed [32*rb (or 32 for the sdf row) x K_l]; the skip layer's
 * K is [rb blocks of h | 2 blocks of gamma]; wt[l] = packed transpose (adjoint / backward).
 * The last Linear is split: w[n_layers-1] = sdf row (1 out-block), w_feat = feature rows.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwSdfNet {
    const void* w[NCW_MAX_LAYERS];
    const float* b[NCW_MAX_LAYERS];
    const void* wt[NCW_MAX_LAYERS];
    const void* w_feat;   /* last layer rows 1..W   [32*rb x 32*rb]        */
    const float* b_feat;
    const void* wt_feat;  /* its transpose                                  */
    int32_t n_layers;     /* number of Linear layers (9 for the 8x256 net)  */
    int32_t skip_layer;   /* index l whose input is cat([h, gamma])/sqrt2, or -1 */
    int32_t rb;           /* hidden width / 32 (2, 8 or 16)                 */
    int32_t multires;     /* 6                                              */
    float scale;          /* SDFNetwork.scale                               */
    int32_t adj_mode;     /* with wt_lo present: 2 = the adjoint sweep's t_l as a hi + lo pair too (rb = 16: see wt_lo below); 0 / 1 = weights only */
    /* Split-precision VALUE path (fp16 mode, W = 256): w_lo[l] = the rounding residuals of w[l] in the same packed layout
     * (NcwPackDesc.residual), or all NULL.  When present, ncw_sdf_infer* and the forward sweep of ncw_sdf_fwd evaluate
     * sdf with activations AND weights as fp16 hi + lo pairs, three MFMAs per product (hi.hi + lo.hi + hi.lo, f32
     * accumulate): ~2^-22 relative, i.e. fp32-like SDF values at fp16 MFMA rate.  sigmoid(sdf * inv_s) multiplies an SDF
     * error by inv_s = exp(10 variance) -- 20 at initialisation, several hundred where NeuS trains (models/neuconw.py:
     * 173-179, rendering/renderer.py:624-632) -- so the 5e-4 of a plain fp16 evaluation is 0.2 in the sigmoid's argument there.
     * The adjoint / backward passes and the feature rows stay plain fp16. */
    const void* w_lo[NCW_MAX_LAYERS];
    /* wt_lo[l] = the rounding residuals of the TRANSPOSED matrices wt[l] (same packed layout), or all NULL.  When present (fp16,
     * W = 256) the analytic adjoint sweep of ncw_sdf_fwd -- the normals -- takes its WEIGHTS as hi + lo pairs (W_hi^T t + W_lo^T t,
     * two MFMAs per product; t stays single fp16): the compositor multiplies the normal's component along the ray by
     * dist * inv_s inside the sigmoid (rendering/renderer.py:600-632), and on trained weights the plain-fp16 adjoint sweep was
     * what put single rays above 1e-4 (scripts/diag/emul_timed_batch.py: worst rays 1.5e-4 -> 3.7e-5).  Forward only: the stash
     * t_l, ncw_sdf_bwd and the weight gradients are unchanged.  adj_mode = 2 (rb = 16, the shipped W = 512): t_l is a hi + lo pair
     * as well (three MFMAs per product, the value chain's accuracy): with 8 + 16 samples per ray one sample carries a ray and
     * the colour network reads ITS normal -- the weights alone as pairs were not enough there (profiles/r06/emul_timed_batch_shipped_tangent*.log). */
    const void* wt_lo[NCW_MAX_LAYERS];
} NcwSdfNet;

/* a-2 `sdf(x)` (neuconw.py:281-282): x [n,3] f32 -> sdf [n] f32.  No grad, last layer 1 row. */
int ncw_sdf_infer(const NcwSdfNet* net, int prec, const float* x, int64_t n, float* sdf, void* stream);

/* Same network evaluated at ray samples x = o[r] + d[r] * z[r,i]  (renderer.py:519-522, 350-352):
 * rays_o, rays_d [R,3], z [R,n] -> sdf [R,n].  Fuses the point generation into the MLP prologue. */
int ncw_sdf_infer_rays(const NcwSdfNet* net, int prec, const float* rays_o, const float* rays_d, const float* z,
                       int R, int n, float* sdf, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point source shared by the fused MLP kernels: explicit points or ray samples (the point
 * generation of renderer.py:586-597 / :176-186 is fused into the MLP prologue).
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwPoints {
    const float* x;            /* mode 0: [n,3] explicit points                              */
    const float* rays_o;       /* modes 1,2: [R,3]                                           */
    const float* rays_d;       /* modes 1,2: [R,3]                                           */
    const float* z;            /* modes 1,2: [R,per_ray]                                     */
    const float* sample_dist;  /* mode 2: [R]                                                */
    int32_t per_ray;
    int32_t mode;              /* 0: x;  1: o + d z;  2: section mid-point o + d (z_i + dist_i/2);
                                  3: regular grid generated on chip (utils/visualization.py:46-50);
                                  4: a SELECTION of the mode-2 points: point k of the launch is ray sample idx[k]
                                     (= ray * per_ray + i), only the first min(n, *count) are processed, outputs
                                     and cotangents stay addressed by the ray sample (dense [R, per_ray] arrays), the
                                     stashes by k (ncw_bg_select; background NeRF kernels at W = 256, 16-bit only) */
    /* mode 3: point p (+ grid_start) of linspace(gmin, gmax, gdim)^3, meshgrid 'ij' (x slowest),
     * mapped to the unit sphere as (x - gorigin) / gradius. */
    float gmin[3], gmax[3], gorigin[3], gradius;
    int32_t gdim;
    int32_t _gpad;
    int64_t gstart;
    const int32_t* idx;        /* mode 4: DEVICE int32[n] ray-sample indices                               */
    const int32_t* count;      /* mode 4: DEVICE int32[1] number of valid entries of idx                  */
} NcwPoints;

/* config 5 (tools/extract_mesh.py / utils/visualization.py:37-85): sdf of `count` points of the regular grid
 * described by pts (mode 3) starting at linear index pts->gstart; no coordinate array ever exists. */
int ncw_sdf_infer_points(const NcwSdfNet* net, int prec, const NcwPoints* pts, int64_t count, float* sdf, void* stream);


/* Activation stash of the SDF net in fragment-native layout [tile32][blocks][4][64 lanes][4]
 * (element = f32 for prec 0, bf16 for prec 1).  HOST struct of device pointers.
 * Written by ncw_sdf_fwd (gamma, h, s, t, feat), ncw_color_bwd (dfeat) and ncw_sdf_bwd
 * (qbar, zbar, zsdf, one); consumed by ncw_sdf_bwd and ncw_wgrad. */
typedef struct NcwSdfStash {
    void* gamma;                 /* encoding, 2 blocks                                        */
    void* h[NCW_MAX_LAYERS];     /* h[l], l>=1: input of layer l = Softplus(z_{l-1}), rb blocks */
    void* s[NCW_MAX_LAYERS];     /* Softplus'(z_l) is recomputed as 1 - exp(-100 h[l+1]): no stash of its own.  fp16 mode with
                                  * NcwSdfNet.adj_mode 2 (rb = 16): s[l], l >= 1 = the fp16 RESIDUALS of h[l] (h_lo = h16(h - h16(h))),
                                  * written by the split value chain and read back by the adjoint sweep of the SAME launch, whose
                                  * phi' = 1 - exp(-100 (h + h_lo)) then carries no fp16 rounding of h; NULL = phi' from h[l] alone */
    void* t[NCW_MAX_LAYERS];     /* t[l] = a_l * s[l] (adjoint pass), l <= L-2                 */
    void* feat;                  /* feature vector z_{L-1}[1:], rb blocks                      */
    void* dfeat;                 /* upstream d(feat), rb blocks                                */
    void* qbar[NCW_MAX_LAYERS];  /* qbar[0]: 2 blocks (J_gamma nbar); qbar[l]: rb blocks       */
    void* zbar[NCW_MAX_LAYERS];  /* zbar[l] = dL/dz_l, l <= L-2                                */
    void* zsdf;                  /* 1 block: feature 0 = d_sdf                                 */
    void* one;                   /* 1 block: feature 0 = 1                                     */
} NcwSdfStash;

/* a-2/a-5 forward of the SDF net WITH its analytic input gradient (neuconw.py:263-296):
 * sdf [n], grad [n,3] (= d sdf / d x), plus the stash for the backward.  One launch.
 * FORWARD-ONLY form (the reference's validation / novel-view render and vertex colours, rendering/renderer.py:785-916
 * under no_grad, :951-961; models/neuconw.py:353-376 called without a backward): pass a stash whose t[0] is NULL.  The
 * outputs are the same bit for bit; of the stash only h[1 .. L-1] (re-read by the adjoint sweep of the SAME launch: it must
 * exist as scratch, W x 2 B per point and layer) and feat (ncw_color_fwd's input) are written -- no gamma, no t. */
int ncw_sdf_fwd(const NcwSdfNet* net, int prec, const NcwPoints* pts, int64_t n, float* sdf, float* grad,
                const NcwSdfStash* stash, void* stream);
/* First- and second-order backward (SURVEY 8a-2 "parameter-gradient specification"): consumes
 * d_sdf [n], d_grad [n,3] and stash->dfeat; fills stash->qbar/zbar/zsdf/one for ncw_wgrad. */
int ncw_sdf_bwd(const NcwSdfNet* net, int prec, const NcwPoints* pts, int64_t n, const float* d_sdf,
                const float* d_grad, const NcwSdfStash* stash, void* stream);

/* ------------------------------------------------------------------------------------------
 * Colour network -- RenderingNetwork, models/neuconw.py:59-170 (encode_apperence, mode "idr").
 *   f  = xyz_encoding_final(feat)                       [rbf x rbf], no activation
 *   e0 = relu(static_linear_0([f | gamma4(dir) | a]))   K = [rbf blocks | AUX1 (3 blocks)]
 *   e_i= relu(static_linear_i(e_{i-1}))                 [rbh x rbh]
 *   x0 = relu(lin0([points | normals | e]))             K = [rbh blocks | AUX2 (1 block: pts, normals)]
 *   x_l= relu(lin_l(x_{l-1})) ... rgb = sigmoid(lin_last(x))
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwColorNet {
    const void* w_f; const void* wt_f; const float* b_f;
    const void* w_e[4]; const void* wt_e[4]; const float* b_e[4];
    const void* w_l[8]; const void* wt_l[8]; const float* b_l[8];
    int32_t n_head;  /* static_head_layers                       */
    int32_t n_lin;   /* trunk Linear count (n_layers + 1)        */
    int32_t rbf, rbh, rbc, n_a;
    /* fp16 mode, FORWARD only: the residual matrices h16(W - h16(W)) of the forward matrices above (packed with
     * NcwPackDesc.residual); NULL = one rounding per weight.  With them ncw_color_fwd evaluates W_hi x + W_lo x: on trained
     * weights the colour network's weight rounding was the largest remaining term of the fp16 mode's colour error
     * (scripts/diag/emul_color16.py: 5 % of the rays above 1e-4 -> none). */
    const void* w_f_lo; const void* w_e_lo[4]; const void* w_l_lo[8];
    /* with the residual matrices present: 1 = the ACTIVATIONS of every layer as fp16 hi + lo pairs too (a third pass W_hi x_lo; rbf
     * 8 / 16 only).  Default at d_feature = 512, the shipped width: with 8 + 16 samples one sample carries a ray and the
     * activations' rounding was, with the normals', what kept rays above 1e-4 on trained weights (ncw_color.hip).  Forward only.
     * At rbf / rbh / rbc = 8 / 4 / 8 the value 1 runs the weights-stationary kernel (csrc/ncw_split.hip color_fwdS_kernel: eight waves per
     * workgroup, the same bits); 2 = the pairs through the generic register-resident kernel, as at every other width (bisecting,
     * tests/test_gpu_color_fwd_ws.py). */
    int32_t act_split;
    int32_t _pad;
} NcwColorNet;

typedef struct NcwColorStash {
    void* aux1;      /* 3 blocks */
    void* aux2;      /* 1 block  */
    void* f;         /* rbf      */
    void* e[4];      /* rbh, post-relu head activations */
    void* x[8];      /* rbc, post-relu trunk activations x[0..n_lin-2] */
    void* zf;        /* rbf : dL/d f (pre-activation of xyz_encoding_final) */
    void* ze[4];     /* rbh */
    void* zx[8];     /* rbc */
    void* zo;        /* 1 block: dL/d(pre-sigmoid rgb), features 0..2 */
    const float* aux_bias; /* NULL, or [R, 32 rbh] fp32 from ncw_aux_ray_bias: the per-ray part of the head's first layer,
                            * W_e0[:, view-dir | appearance columns] . [gamma_4(d) | a], added to that layer's bias in the
                            * FORWARD instead of being multiplied from 16-bit operands (the backward is unchanged) */
} NcwColorStash;

/* normals [n,3] (the SDF gradient), a [R or n, n_a] appearance rows indexed by the point's ray,
 * feat: stash (rbf blocks) written by ncw_sdf_fwd  ->  rgb [n,3].
 * FORWARD-ONLY form: a stash whose aux1 is NULL (aux_bias stays an input): the same rgb bit for bit, nothing is stored. */
int ncw_color_fwd(const NcwColorNet* net, int prec, const NcwPoints* pts, int64_t n, const float* normals,
                  const float* a, const void* feat_stash, float* rgb, const NcwColorStash* stash, void* stream);
/* d_rgb [n,3] -> d_grad[n,3] += d(normals), d_a [R,n_a] += (atomics; zero it first), dfeat stash (rbf),
 * d_a_rows: NULL, or [n,n_a] -- then every point's appearance-code adjoint is STORED as its row instead of being
 * added to d_a with atomics, and ncw_ray_sum_rows reduces the rows of a ray in sample order (reproducible; the
 * fp32 parity mode uses it).
 * and the z-stashes for ncw_wgrad.
 * Both return, without a launch, NCW_E_UNSUPPORTED for NcwPoints mode 4 and NCW_E_BADARG for prec = f32 with w_f_lo set. */
int ncw_color_bwd(const NcwColorNet* net, int prec, const NcwPoints* pts, int64_t n, const float* rgb,
                  const float* d_rgb, float* d_grad, float* d_a, float* d_a_rows, void* dfeat_stash,
                  const NcwColorStash* stash, void* stream);

/* ------------------------------------------------------------------------------------------
 * Background NeRF -- models/nerf.py:86-183 (use_viewdirs, encode_appearance) evaluated on the
 * inverted-sphere points of renderer.py:176-186 (fused into the prologue).
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwNerfNet {
    const void* w_p[8]; const void* wt_p[8]; const float* b_p[8];
    const void* w_alpha; const void* wt_alpha; const float* b_alpha;
    const void* w_feat; const void* wt_feat; const float* b_feat;
    const void* w_a[4]; const void* wt_a[4]; const float* b_a[4];
    const void* w_rgb; const void* wt_rgb; const float* b_rgb;
    int32_t D;       /* trunk depth (8)                                         */
    int32_t skip;    /* layer index after whose ReLU gamma(p) is concatenated    */
    int32_t rbn, rbh, n_head, n_a;
    /* fp16 mode: the rounding residuals h16(W - h16(W)) of the FORWARD matrices above (NcwPackDesc.residual), or all NULL: the
     * operands of ncw_nerf_refine. */
    const void* w_p_lo[8]; const void* w_alpha_lo; const void* w_feat_lo; const void* w_a_lo[4]; const void* w_rgb_lo;
} NcwNerfNet;

typedef struct NcwNerfStash {
    void* gp;        /* 3 blocks: gamma_10(p4) (84)    */
    void* aux1;      /* 3 blocks                        */
    void* h[9];      /* h[i], i=1..D: post-relu trunk   */
    void* featn;     /* rbn: feature_linear output      */
    void* e[4];      /* rbh                             */
    void* zp[8];     /* rbn: dL/dz of trunk layer i     */
    void* zalpha;    /* 1 block: feature 0 = d density  */
    void* zfeat;     /* rbn                             */
    void* ze[4];     /* rbh                             */
    void* zrgb;      /* 1 block: features 0..2          */
    const float* aux_bias; /* NULL, or [R, 32 rbh] fp32 from ncw_aux_ray_bias (as NcwColorStash.aux_bias): the per-ray part of
                            * apperence_encoding.static_linear_0 (models/nerf.py:131-139,173-174), forward only */
} NcwNerfStash;

/* pts: mode 2 on z_feed (section mid-points, inverted-sphere reparametrisation applied inside), or
 * x4 != NULL: explicit [n,4] points with pts->rays_d / a indexed per point (NeRF.forward API).
 * -> density [n] (raw), rgb [n,3] (raw, no sigmoid).
 * FORWARD-ONLY form: a stash whose gp is NULL (aux_bias stays an input): the same outputs bit for bit, nothing is stored. */
int ncw_nerf_fwd(const NcwNerfNet* net, int prec, const NcwPoints* pts, const float* x4, int64_t n, const float* a,
                 float* density, float* rgb, const NcwNerfStash* stash, void* stream);
int ncw_nerf_bwd(const NcwNerfNet* net, int prec, const NcwPoints* pts, int64_t n, const float* d_density,
                 const float* d_rgb, float* d_a, float* d_a_rows, const NcwNerfStash* stash, void* stream);
/* FORWARD REFINEMENT of the background NeRF in split precision (fp16 mode, W = 256; models/nerf.py:156-182 on the points of
 * rendering/renderer.py:176-186): density / raw rgb of the SELECTED samples (pts: NcwPoints mode 4, the list of ncw_bg_select --
 * the samples whose background the compositor can use) are re-evaluated with gamma_10(p4), weights (net->w_*_lo) and hidden
 * activations as fp16 hi + lo pairs (three MFMAs per product, f32 accumulate: fp32-level outputs) and written over the
 * plain-fp16 results of ncw_nerf_fwd at those samples.  aux_bias: the per-ray fp32 rows of ncw_aux_ray_bias ([R, 128]) -- the
 * view-direction / appearance-code columns of the head.  Forward only (the stash and the backward are the plain launch's).
 * Rays whose colour is all background carry the plain NeRF's error undiluted: 1.1e-4 .. 1.6e-4 on trained weights without this. */
int ncw_nerf_refine(const NcwNerfNet* net, int prec, const NcwPoints* pts, int64_t n, const float* aux_bias, float* density,
                    float* rgb, void* stream);
/* Batch assembly from the HBM-resident ray cache.  Replaces, per batch, PhototourismDataset.__getitem__
 * for split "train" (datasets/phototourism.py:709-726: rays = row[0:8] ++ row[10:13] (with semantics) / row[9:12],
 * ts = long(row[8]), semantics = row[9]), the DataLoader's collate + pinned H2D copy, and the black-list test of
 * NeuconWSystem.training_step (lightning_modules/neuconw_system.py:345-349): keep[b] = 0 iff label[b] is one of
 * mask_ids (<= 4 ids; the shipped RAY_MASK_LIST has 4).  all_rays [n_rows, ncols] (ncols 13 with semantics, 12 without),
 * all_rgbs [n_rows,3], idx [B] int64 or NULL (= identity); outputs rays [B,11], ts [B] i64, label [B] i64 or NULL,
 * rgbs [B,3] or NULL, keep [B] u8 or NULL.  mask_ids is a HOST array. */
int ncw_batch_assemble(const float* all_rays, int ncols, const float* all_rgbs, const int64_t* idx, int64_t n_rows,
                       int64_t B, int with_semantics, float* rays, int64_t* ts, int64_t* label, float* rgbs,
                       const int* mask_ids, int n_ids, uint8_t* keep, void* stream);
/* ------------------------------------------------------------------------------------------
 * Per-step glue of render() / the loss as single launches (each replaces 6-25 tiny torch kernels; the step is
 * GPU-bound, so every 3-5 us launch counts).
 * ---------------------------------------------------------------------------------------- */
/* models/neuconw.py:131-140: out[r, j] = sum_k w[j, col0 + k] * [gamma_4(rays_d[r]) (27) | a[r] (n_a)][k], fp32, once per RAY
 * (w: the row-major fp32 weight of static_linear_0, row stride ldw; out row stride ldo >= n_out).  The appearance code and
 * the view direction are per-ray constants: their fp16 rounding is coherent along a ray and was the largest term of the fp16
 * mode's colour error on trained weights (scripts/diag/emul_color16.py). */
int ncw_aux_ray_bias(const float* w, int ldw, int col0, int n_out, const float* rays_d, const float* a, int n_a, int64_t R,
                     float* out, int ldo, void* stream);
/* renderer.py:793-806: rays [R,ncols >= 8] -> rays_o = (rays[:,0:3] - origin) / radius, rays_d = rays[:,3:6],
 * near = rays[:,6] / radius, far = rays[:,7] / radius, depth_gt = rays[:,8] / radius, depth_weight = rays[:,9]
 * (zeros when ncols < 10).  origin: HOST float[3]. */
int ncw_ray_prologue(const float* rays, int ncols, int64_t R, const float* origin_host, float radius, float* rays_o,
                     float* rays_d, float* near, float* far, float* depth_gt, float* depth_weight, void* stream);
/* SingleVarianceNetwork (models/neuconw.py:173-179) as used by render_core (renderer.py:624-632):
 * inv_s = clamp(exp(10 variance), 1e-6, 1e6), s_val = 1 / inv_s; backward: d_variance = 10 inv_s [1e-6 < inv_s < 1e6]
 * sum_r d_inv_s[r] (the per-ray terms of ncw_composite_bwd, summed in a fixed order). */
int ncw_inv_s_fwd(const float* variance, float* inv_s, float* s_val, void* stream);
int ncw_inv_s_bwd(const float* d_inv_s_rays, int64_t R, const float* inv_s, float* d_variance, void* stream);
/* NeuconWLoss (losses.py:21-43): loss = coef * ( sum|color - rgbs| / (R + 1e-5) + igr_w * gradient_error
 *   + mask_w * mean(mask_error[n_mask]) + depth_w * mean(sfm[n_sfm]) ); NULL / 0 switches a term off.
 * bwd: d_color [R,3], d_gradient_error [1], d_mask_error [n_mask], d_sfm [n_sfm] for an upstream d_loss [1]. */
int ncw_loss_fwd(const float* color, const float* rgbs, int64_t R, const float* gradient_error, const float* mask_error,
                 int64_t n_mask, const float* sfm, int64_t n_sfm, float coef, float igr_w, float mask_w, float depth_w,
                 float* loss, void* stream);
int ncw_loss_bwd(const float* d_loss, const float* color, const float* rgbs, int64_t R, int64_t n_mask, int64_t n_sfm,
                 float coef, float igr_w, float mask_w, float depth_w, float* d_color, float* d_gradient_error,
                 float* d_mask_error, float* d_sfm, void* stream);
/* out[idx[r], :] += rows[r, :] with f32 atomics (out [n_out, n_cols], zero-filled or accumulating; indices outside
 * [0, n_out) are skipped): the backward of the appearance-embedding lookup `embeddings["a"](ts)` (renderer.py:808). */
int ncw_scatter_add_rows(const float* rows, const int64_t* idx, int64_t R, int n_cols, int64_t n_out, float* out,
                         void* stream);
/* out[R,n_cols] (+)= per-ray sums of rows[R*per_ray, n_cols] in sample order (see d_a_rows above). */
int ncw_ray_sum_rows(const float* rows, int64_t R, int per_ray, int n_cols, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight-gradient GEMMs: dense[32*rbx, ld] (f32, forward orientation) += X^T Y over all points,
 * X, Y in stash layout; optional dbias[32*rbx] += column sums of X.  Batched: one launch runs a
 * device table of products (split-K + f32 atomics).
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwWgradDesc {
    const void* x;     /* stash, rbx blocks  (output-feature side)  */
    const void* y;     /* stash, rby blocks  (input-feature side)   */
    float* dense;      /* [32*rbx, ld] (+ column offset already applied) */
    float* dbias;      /* [32*rbx] or NULL                           */
    int32_t rbx, rby, ld;
    int32_t ksplit;    /* ncw_wgrad_tiled only: > 0 overrides the launch-wide split-K for this product */
    int64_t n_points;  /* ncw_wgrad_tiled only: > 0 overrides the launch-wide point count            */
    const int32_t* n_points_dev; /* every entry point: DEVICE int32[1] or NULL (a selection made on the device, NcwPoints
                                  * mode 4).  The kernels work in whole tiles of 32 points: the product covers the tiles
                                  * [0, ceil(min(n_points, *n_points_dev) / 32)) of its stashes, all 32 lanes of the last one
                                  * included, so X must be ZERO in the padded lanes of that tile (the producers write their
                                  * cotangents there as zero; Y may hold anything finite); the K-slices re-divide those tiles */
} NcwWgradDesc;
/* descs: DEVICE array; wg_prefix: device int32[n_desc+1] exclusive prefix of
 * ceil(rbx/4)*ceil(rby/4)*ksplit workgroups per product; total_wgs = wg_prefix[n_desc]. */
int ncw_wgrad(const NcwWgradDesc* descs, const int32_t* wg_prefix, int n_desc, int total_wgs, int ksplit,
              int prec, int64_t n_points, void* stream);
/* Run-to-run reproducible variant (the fp32 parity mode uses it): every K-slice writes its 128 x 128 partial into its
 * own slab of `partials` (DEVICE scratch of ncw_wgrad_ordered_scratch_floats(total_wgs) floats, contents
 * irrelevant on entry) and a second launch adds the slabs of a quadrant in slice order.  The autograd GEMMs it
 * replaces (torch `mm` backward of F.linear, models/neuconw.py:269-278) are deterministic on the reference's CPU path. */
int64_t ncw_wgrad_ordered_scratch_floats(int total_wgs);
int ncw_wgrad_ordered(const NcwWgradDesc* descs, const int32_t* wg_prefix, int n_desc, int total_wgs, int ksplit,
                      int prec, int64_t n_points, float* partials, void* stream);
/* bf16 only, explicit workgroup tile: tile 0 = 128 x 256 features (wg_prefix counts ceil(rbx/4)*ceil(rby/8)*ksplit),
 * tile 1 = 256 x 256 (ceil(rbx/8)*ceil(rby/8)*ksplit): every stash element is read once per product.
 * A product's own ksplit / n_points (when > 0) replace the launch-wide values, so products of different
 * networks and sizes share ONE launch with a work-proportional split. */
int ncw_wgrad_tiled(const NcwWgradDesc* descs, const int32_t* wg_prefix, int n_desc, int total_wgs, int ksplit,
                    int tile, int64_t n_points, void* stream);
/* the same for fp16 stashes (prec NCW_PREC_F16; ncw_wgrad / ncw_wgrad_ordered take it through `prec`) */
int ncw_wgrad_tiled_f16(const NcwWgradDesc* descs, const int32_t* wg_prefix, int n_desc, int total_wgs, int ksplit,
                        int tile, int64_t n_points, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser step over flat fp32 buffers (16-byte aligned): global-norm clip + Adam in one launch.
 * Replaces torch.nn.utils.clip_grad_norm_ (train.py:61) + torch.optim.Adam(eps=1e-7).step()
 * (utils/__init__.py:23-31) for parameters re-seated into one flat buffer:
 *   coef = total_norm ? min(max_norm / (total_norm[0] + 1e-6), 1) : 1;   g *= coef  (written back)
 *   m += (1-beta1)(g - m);  v = beta2 v + (1-beta2) g g;
 *   p -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller.
 * total_norm: DEVICE scalar (the 2-norm of grad) or NULL for no clipping.  A non-finite total_norm skips the step
 * (nothing is written): one overflowed fp16 step must not poison the parameters and the moments.
 * ---------------------------------------------------------------------------------------- */
int ncw_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float step_size,
                  float beta1, float beta2, float eps, float bias_correction2_sqrt, const float* total_norm,
                  float max_norm, void* stream);

/* The same update with every step-dependent quantity on the DEVICE (trainer.FlatAdam): `state` holds the applied-step
 * counter and the scalars derived from it, so a skipped step does not advance Adam's bias correction, nothing is a
 * per-step kernel argument (HIP-graph capturable), and the fp16 loss scale adapts without a device->host round trip.
 * Two launches: a one-thread prologue that reads total_norm (device scalar or NULL) and updates `state` / `loss_scale`,
 * then the elementwise update.
 *   finite norm:  step += 1; coef = max_norm > 0 ? min(max_norm / (norm + 1e-6), 1) : 1; step_size = lr / (1 - beta1^step)
 *                 and bc2_sqrt = sqrt(1 - beta2^step) in double; after `growth_interval` consecutive finite steps the loss
 *                 scale doubles (<= scale_max);
 *   non-finite:   nothing is written to param / grad / moments, step stays, skipped += 1, the loss scale halves (>= scale_min).
 * loss_scale: device float[2] = {scale, 1 / scale} (read by NcwCompositeGrad.grad_scale_dev / NcwUnpackDesc.grad_mul_dev) or
 * NULL; growth_interval 0 = never grow.  lr_dev: device scalar overriding `lr` (schedulers under graph replay) or NULL.
 * The reference's recipe has no counterpart for the scale (fp32 training, train.py:48-62). */
/* total_norm of torch.nn.utils.clip_grad_norm_ (train.py:61) over ONE flat fp32 buffer (16-byte aligned): norm[0] = ||grad||_2.
 * One launch, fixed summation order (run-to-run reproducible), non-finite entries propagate.  scratch: device floats,
 * ncw_grad_norm_scratch_floats() of them; it holds the partial sums and the blocks' arrival ticket, which a stream-ordered memset
 * arms in front of every launch (capture-safe).  One scratch buffer serves ONE stream at a time. */
int64_t ncw_grad_norm_scratch_floats(void);
int ncw_grad_norm(const float* grad, int64_t n, float* scratch, float* norm, void* stream);

typedef struct NcwAdamState {
    int32_t step;      /* applied (non-skipped) steps: Adam's t */
    int32_t good;      /* consecutive finite steps since the last scale change */
    int32_t skipped;   /* total skipped steps */
    int32_t skip_now;  /* 1: the step being applied was skipped */
    float coef, step_size, bc2_sqrt, last_norm;
} NcwAdamState;
int ncw_adam_step_dev(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, NcwAdamState* state,
                      const float* total_norm, float lr, const float* lr_dev, float beta1, float beta2, float eps,
                      float max_norm, float* loss_scale, int growth_interval, float scale_min, float scale_max,
                      void* stream);

/* Layout converters between row-major f32 [n, F] and the stash layout (rb = ceil(F/32) blocks,
 * element type by prec).  Used at the module boundary (NeuconW.forward returning feature vectors,
 * tests); padded lanes / features are written as zero. */
int ncw_stash_from_rows(int prec, const float* rows, int64_t n, int F, int rb, void* stash, void* stream);
int ncw_stash_to_rows(int prec, const void* stash, int64_t n, int F, int rb, float* rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-ray sampler kernels (one wavefront per ray).  All arrays f32, row-major [R, n].
 * ---------------------------------------------------------------------------------------- */
/* renderer.py:488-514: coarse z (+ optional whole-ray jitter rand_shift[R]), inverse-depth outside
 * samples (+ optional stratified jitter rand_out[R,O]), sample_dist.  rand_* may be NULL. */
int ncw_sample_coarse(const float* near, const float* far, const float* s_near, const float* s_far, int R,
                      int n_samples, int n_outside, const float* rand_shift, const float* rand_out,
                      float* z, float* z_out, float* sample_dist, void* stream);
/* renderer.py:257-341 (up_sample) + :15-48 (sample_pdf, det=True): -> z_new [R, n_new] */
int ncw_upsample(const float* rays_o, const float* rays_d, const float* z, const float* sdf, int R, int n,
                 float inv_s, int n_new, float* z_new, void* stream);
/* renderer.py:343-363, :566, :835-836: stable sort of cat([a,b]) per ray, optional payload
 * (pa/pb/pout may be NULL). */
int ncw_sort_merge(const float* a, int na, const float* b, int nb, const float* pa, const float* pb, int R,
                   float* out, float* pout, void* stream);
/* renderer.py:549-565 boundary samples: zb [R, nb] (unsorted; feed to ncw_sort_merge) */
int ncw_boundary(const float* near, const float* far, const float* z, int n, int R, int nb, float* zb,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Voxel guidance (config 3): native replacement of kaolin's SPC ray tracing used by
 * tools/prepare_data/generate_voxel.py:311-439 / renderer.py:380-456.  Occupancy = bit-packed dense
 * grid of side 2^level over [-1,1]^3 (x slowest) + 8^3-brick mask.  3 <= level <= 10.
 * ---------------------------------------------------------------------------------------- */
/* set the voxels containing the given normalised points (atomicOr; occ/brick must be zeroed first):
 * occ  uint32[(2^level)^3 / 32], brick uint32[ceil((2^level / 8)^3 / 32)] */
int ncw_voxel_build(const float* pts_normalised, int64_t n, int level, uint32_t* occ, uint32_t* brick, void* stream);
/* per ray: entry depth (SfM units) of the first / last occupied voxel; 0 where the ray misses or
 * near <= 1e-4 (generate_voxel.py:397).  scene_origin_host: HOST float[3]. */
int ncw_ray_voxel_near_far(const float* rays_o_sfm, const float* rays_d, int R, const float* scene_origin_host,
                           float scale, int level, const uint32_t* occ, const uint32_t* brick, float* near_sfm,
                           float* far_sfm, void* stream);
/* kaolin.render.spc.unbatched_raytrace(octree, points, pyramid, prefix, origin, direction, level, return_depth=True,
 * with_exit=...) as tools/prepare_data/generate_voxel.py:358-368 calls it: EVERY intersection of a ray with an occupied
 * level-`level` voxel (a "nugget"), ordered by ray, then by depth.  Origins are already normalised to the cube [-1,1]^3
 * (generate_voxel.py:345) and nothing is added to them.  Two calls: offsets == NULL writes counts[R] (nuggets per ray); with
 * offsets[R] (their exclusive prefix sum) ray r writes nug_ray / nug_voxel (linear index (x 2^level + y) 2^level + z) /
 * nug_depth [N,2] = (entry, exit) depth along the direction as given, from offsets[r] on.  (compat/kaolin maps the voxel
 * index to kaolin's point-hierarchy index.) */
int ncw_ray_voxel_trace(const float* rays_o_norm, const float* rays_d, int R, int level, const uint32_t* occ,
                        const uint32_t* brick, const int32_t* offsets, int32_t* counts, int32_t* nug_ray,
                        int32_t* nug_voxel, float* nug_depth, void* stream);

/* ------------------------------------------------------------------------------------------
 * Compositor: renderer.py:205-216 (background alpha) + :586-783 (render_core after the networks).
 * HOST structs of device pointers.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwCompositeIn {
    const float* rays_o;       /* [R,3] unit-sphere units                         */
    const float* rays_d;       /* [R,3]                                           */
    const float* z;            /* [R,S] sorted inside samples                     */
    const float* z_feed;       /* [R,S+O] sort(cat(z, z_out)) or NULL (no bg)     */
    const float* sample_dist;  /* [R]                                             */
    const float* sdf;          /* [R,S]                                           */
    const float* grad;         /* [R,S,3] d sdf / d x                             */
    const float* rgb;          /* [R,S,3]                                         */
    const float* density;      /* [R,S+O] raw NeRF density or NULL                */
    const float* bg_rgb;       /* [R,S+O,3] or NULL                               */
    const float* inv_s;        /* [1] device scalar exp(10 variance)              */
    const float* background_rgb; /* [3] or NULL                                   */
    const float* cos_anneal_dev; /* [1] device scalar or NULL: when set it replaces cos_anneal (so that a
                                    captured HIP graph of the step can be replayed with a new ratio)  */
    float cos_anneal;
    int32_t R, S, O, has_bg, trim_sphere;
} NcwCompositeIn;

typedef struct NcwCompositeOut {
    float* color;        /* [R,3] */
    float* color_sphere; /* [R,3] */
    float* color_bg;     /* [R,3] */
    float* weights;      /* [R,S+O] */
    float* weights_sum;  /* [R]   */
    float* cdf;          /* [R,S] prev_cdf */
    float* inside;       /* [R,S] */
    float* depth;        /* [R]   */
    float* normals;      /* [R,3] */
    float* eik;          /* [2,R] per-ray eikonal partials: row 0 = sum relax*(|g|-1)^2, row 1 = sum relax */
    float* mid_z;        /* [R,S] */
    float* dists;        /* [R,S] */
    float* bg_alpha;     /* [R,S+O] or NULL when !has_bg */
    float* weights_max;  /* [R] max of weights over the ray (render()'s "weights_max", renderer.py:905) or NULL */
} NcwCompositeOut;

typedef struct NcwCompositeGrad {
    const float* d_color;       /* [R,3] upstream */
    const float* d_weights_sum; /* [R]            */
    const float* d_depth;       /* [R]            */
    const float* d_eik_num;     /* [R]            */
    float* d_sdf;      /* [R,S]     */
    float* d_grad;     /* [R,S,3]   */
    float* d_rgb;      /* [R,S,3]   */
    float* d_density;  /* [R,S+O]   */
    float* d_bg_rgb;   /* [R,S+O,3] */
    float* d_inv_s;    /* [R]: every ray's term of d loss / d inv_s; the caller sums them (order-fixed) */
    float grad_scale;  /* multiplies every upstream cotangent on load (0 = 1): the fp16 mode's loss scale, so that the
                        * per-point adjoints the MLP backward kernels round to fp16 stay in its normal range; the caller
                        * divides it back out of the parameter gradients (NcwUnpackDesc.scale), d_a and d_inv_s */
    const float* grad_scale_dev; /* device scalar multiplied on top of grad_scale (the dynamic loss scale) or NULL */
    const float* d_normals;      /* [R,3] upstream or NULL: cotangent of NcwCompositeOut.normals (the floor-normal loss);
                                  * NULL runs the kernel without its two terms (the same program as before the field existed) */
} NcwCompositeGrad;

/* Dead-background elimination (renderer.py:637,693-708 with trim_sphere): the background NeRF's density / colour in
 * column i < S of the [R, S + O] background arrays is multiplied by 1 - inside_sphere[i] in the compositor, forward and
 * backward, where inside_sphere[i] belongs to PRIMARY sample i (section mid-point of z [R, S], the last section ending
 * sample_dist further) -- an index pairing, wherever the i-th point of z_feed lies; only the other columns need the NeRF
 * at all.  Writes the ray-sample indices (r * M + i, M = S + O, ray-major, ascending) of the columns to evaluate -- i < S
 * with inside_sphere[i] == 0 and every i >= S (the n_outside samples) -- into idx[R * M], the exclusive prefix of the
 * per-ray counts into ray_offsets[R + 1] and their number into count[1]. */
int ncw_bg_select(const float* rays_o, const float* rays_d, const float* z, const float* sample_dist, int R, int S,
                  int O, int32_t* idx, int32_t* ray_offsets, int32_t* count, void* stream);

int ncw_composite_fwd(const NcwCompositeIn* in, const NcwCompositeOut* out, void* stream);
int ncw_composite_bwd(const NcwCompositeIn* in, const NcwCompositeGrad* g, void* stream);

/* Per-ray loss terms that render() itself returns (renderer.py:763-765 gradient_error, :869-877 mask_error,
 * :892-897 sfm_depth_loss) and their backward.  All arrays [R] f32 (label int64, NULL = no masking);
 * mask_ids (HOST, <= 4 ids): labels whose rays get mask 0.  mask_error / sfm_depth_loss may be NULL (term off).
 * sfm_depth_loss is the sync-free form (depth-gt)^2 w [w>0] R / max(#{w>0},1): its mean over R equals the
 * reference's mean over the selected rays.  scalars: DEVICE float[3] = {gradient_error, sum(eik_den), count}. */
int ncw_ray_tail_fwd(const float* weights_sum, const int64_t* label, const int* mask_ids, int n_ids,
                     const float* depth, const float* depth_gt, const float* depth_weight, const float* eik_num,
                     const float* eik_den, int R, float* mask_error, float* sfm_depth_loss, float* scalars,
                     void* stream);
/* cotangents may be NULL (treated as zero); writes d_weights_sum, d_depth, d_eik_num [R] */
int ncw_ray_tail_bwd(const float* weights_sum, const int64_t* label, const int* mask_ids, int n_ids,
                     const float* depth, const float* depth_gt, const float* depth_weight, int R,
                     const float* scalars, const float* d_mask_error, const float* d_sfm_depth_loss,
                     const float* d_gradient_error, float* d_weights_sum, float* d_depth, float* d_eik_num,
                     void* stream);

/* The floor-normal term of render() (renderer.py:918-945 floor_loss) and its backward.  floor[r] = label[r] (int64) is one of
 * floor_ids (HOST, <= 4 ids); n_gt (HOST): the unit floor normal in SfM coordinates.
 *   floor_error[r,:] = |normals[r,:] - n_gt| * floor[r] * (scaled ? R / max(n_floor, 1) : 1)       [R,3]
 *   scalars: DEVICE float[2] = {n_floor, y_var}; y_var = unbiased variance over the 3 n_floor coordinates of
 *            rays_o + rays_d * depth on the floor rays (0 when there is none)
 * scaled = 1 is the sync-free form: the mean over all R rows equals the reference's mean over the floor rows.
 * One workgroup, order-fixed sums (no atomics): bitwise reproducible. */
int ncw_ray_floor_fwd(const float* normals, const int64_t* label, const int* floor_ids, int n_ids, const float n_gt[3],
                      const float* rays_o, const float* rays_d, const float* depth, int R, int scaled,
                      float* floor_error /*[R,3]*/, float* scalars /*[2]*/, void* stream);
/* d_normals [R,3] = d_floor_error * sign(normals - n_gt) * floor * scale, sign(0) = 0; scalars as written by the forward */
int ncw_ray_floor_bwd(const float* normals, const int64_t* label, const int* floor_ids, int n_ids, const float n_gt[3],
                      int R, int scaled, const float* scalars, const float* d_floor_error /*[R,3]*/,
                      float* d_normals /*[R,3]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Iso-surface extraction: replaces `skimage.measure.marching_cubes(sdf, level, mask=...)` of
 * utils/visualization.py:114 by MARCHING CUBES on the same grid: one vertex per sign-changing grid edge at its linear
 * zero crossing (the vertex rule of every marching-cubes variant), triangles per cube from the 256-entry case tables
 * generated by neuralrecon-w_amd/mc_tables.py (tri [256][16] int8 edge triples, -1 padded; ntri [256]; edges [12][2]
 * corner pairs; corner k = offset (k&1, k>>1&1, k>>2&1), configuration bit k = value < level).  skimage's triangulation of
 * the ambiguous configurations is not reproducible without skimage: the vertex set and the geometry are what is pinned.
 * sdf: [Dx,Dy,Dz] f32 (x slowest).  mask: uint8 [Dx,Dy,Dz] or NULL; the cube with minimum corner (i,j,k) is processed
 * iff mask[i+1,j+1,k+1] (utils/visualization.py:103-112 builds the mask that way).
 *   ncw_mc_count: counts[(Dx-1)(Dy-1)(Dz-1)] int32 triangles per cube (cube index x slowest)
 *   ncw_mc_emit : offsets = EXCLUSIVE prefix sum of counts (int64); writes tri_pos [T,3,3] f32 in grid-index
 *                 coordinates and tri_key [T,3] int64 vertex ids (lo_point * Dx*Dy*Dz + hi_point: weld by key).
 *                 Faces are wound so that normals point towards increasing values.
 * ---------------------------------------------------------------------------------------- */
int ncw_mc_count(const float* sdf, const uint8_t* mask, int Dx, int Dy, int Dz, float level, const int32_t* ntri,
                 int32_t* counts, void* stream);
int ncw_mc_emit(const float* sdf, const uint8_t* mask, int Dx, int Dy, int Dz, float level, const int8_t* tri,
                const int32_t* ntri, const int32_t* edges, const int64_t* offsets, float* tri_pos, int64_t* tri_key,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * Marching cubes on brick-blocked sparse values (csrc/ncw_mc_sparse.hip; mesh.isosurface_sparse): the same surface as
 * ncw_mc_count / ncw_mc_emit under the all-8-corners mask of the sparse mode, without any array of the size of the lattice.
 *   bricks [n,3] int32: the occupied coarse voxels of a [G]^3 lattice, STRICTLY ASCENDING lexicographically in (x, y, z) and
 *                       inside [0, G) (device data: the caller's contract, mesh.isosurface_sparse checks it; whatever the
 *                       list holds, no kernel reads or writes outside its arrays);
 *   up                : sub-voxels per side of a brick, a power of two in 1..32; the fine lattice has side D = G * up <= 16384;
 *   values [K] f32    : K = n * up^3 <= 2^31 - 1, brick-major, then local x, y, z with z fastest (gen_grid_spc's order).
 * A cube is used iff all 8 of its corners are among the K points; corners across an upper face of a brick come from the up to
 * 7 upper neighbour bricks.  Shared with the dense path (csrc/ncw_mc.h): the cube, the configuration test and the edge
 * interpolation, so a vertex has the same bits on both.
 *   ncw_mcs_neighbors: nbr [n,7] int32: entry o - 1 (o = 1..7; bit0 = +x, bit1 = +y, bit2 = +z) = index of the brick at that
 *                      offset, -1 where it is absent or outside the lattice (binary search in the ascending list).
 *   ncw_mcs_count    : counts [K] uint8 = triangles (0..5) of the cube whose minimum corner is sub-voxel i, 0 for an unused cube.
 *   ncw_mcs_cube_ids : sub [M] int64 = indices into counts (the caller's compaction of the non-empty cubes);
 *                      ids [M] int64 = global grid point id (x * D + y) * D + z of each cube's minimum corner.  Sorting by it
 *                      gives the dense path's cube order (x slowest).
 *   ncw_mcs_emit     : sub [M] in that order, offsets [M] int64 = EXCLUSIVE prefix sum of their counts, T = the total; writes
 *                      tri_pos [T,3,3] f32 in fine grid-index coordinates and tri_key [T,3] int64 = lo_point * 3 + a (a = 0, 1, 2
 *                      for the edge along z, y, x): it sorts as the dense key lo_point * n_points + hi_point does and cannot
 *                      overflow.  Winding as ncw_mc_emit.  One lane per output element, no atomics: bitwise reproducible.
 * All return NCW_E_BADARG without a launch for up not a power of two in 1..32, n < 0, K > 2^31 - 1, n_values != K, G < 1,
 * G * up > 16384 (ncw_mcs_neighbors: G > 16384, n > 2^31 - 1), M outside [0, K], T outside [0, 5 M] or a missing pointer; 0
 * without a launch for n == 0 (neighbors, count) or M == 0 (cube_ids, emit).
 * ---------------------------------------------------------------------------------------- */
int ncw_mcs_neighbors(const int32_t* bricks, int64_t n, int G, int32_t* nbr, void* stream);
int ncw_mcs_count(const float* values, int64_t n_values, const int32_t* bricks, const int32_t* nbr, int64_t n, int up, int G,
                  float level, const int32_t* ntri, uint8_t* counts, void* stream);
int ncw_mcs_cube_ids(const int32_t* bricks, int64_t n, int up, int G, const int64_t* sub, int64_t M, int64_t* ids, void* stream);
int ncw_mcs_emit(const float* values, int64_t n_values, const int32_t* bricks, const int32_t* nbr, int64_t n, int up, int G,
                 float level, const int8_t* tri, const int32_t* ntri, const int32_t* edges, const int64_t* sub,
                 const int64_t* offsets, int64_t M, int64_t T, float* tri_pos, int64_t* tri_key, void* stream);


/* ------------------------------------------------------------------------------------------
 * Exact 1-nearest-neighbour search for the mesh evaluation: replaces the per-point
 * `scipy.spatial.KDTree.query` loop of utils/eval_utils.py:126-154 (`nn_correspondance`, the use_o3d=False path of
 * utils/eval_mesh.py:48-123).  Uniform grid of cubic cells over a box chosen by the caller, for the reference cloud
 * P [M,3] and the queries Q [N,3] (f32, recentred by the caller); points and queries outside the box are clamped into the
 * boundary cells (exact all the same: boundary faces never bound the search); cell (cx, cy, cz) =
 * clamp(floor((x - lo) * inv_h), 0, dim - 1), linear key
 * (cx * dim[1] + cy) * dim[2] + cz.  Distances are Euclidean, d^2 = dx*dx + dy*dy + dz*dz; ties on equal d^2 go to the
 * smaller index (= argmin of the brute-force distance matrix).  No approximation, no truncation radius.
 *   ncw_nn_cell_keys  : keys[n] int32 of n points.
 *   ncw_nn_cell_ranges: after a stable sort of P's keys (sorted_keys[m], order[m] = the permutation): cell_range
 *                       [dim0*dim1*dim2][2] int32 (ZEROED by the caller) gets [start, end) of every non-empty cell;
 *                       pts_sorted [m][4] f32 = P in cell order with the original index in .w (int bits).
 *   ncw_nn_query      : q_order = Q in cell order (stable sort of Q's keys); per query dist[n] f32 / idx[n] int64 at the
 *                       query's original position, by Chebyshev shells around its cell, stopping after shell r when
 *                       best d^2 < (b - margin)^2 (b = distance to the faces of the (2r+1)^3 block not on the grid boundary)
 *                       or when the block covers the grid.  Queries still open after `max_shell` shells are appended to
 *                       escaped[] (their count in *n_escaped, zeroed by the caller) and left unwritten.
 *   ncw_nn_brute      : the escaped queries against all of P; scratch uint64[n_esc].
 * NEAREST POINT WITHIN A RADIUS (one launch per query set: no escape list, no brute-force pass):
 *   ncw_nn_coarse     : from the cell_range of a built grid, coarse[c0*c1*c2] int32 = the number of points in every block
 *                       of B^3 fine cells (B a power of two in [1, 65536]; c_a = ceil(dim[a] / B); block (bx, by, bz) at
 *                       (bx * c1 + by) * c2 + bz).  Integer work only.
 *   ncw_nn_query_within: the inputs of ncw_nn_query plus that table, B and max_dist.  With r2 = max_dist * max_dist (one
 *                       float32 product, formed by this entry) and (d2, i) = the minimum of dx*dx + dy*dy + dz*dz over ALL of P
 *                       with ties to the smaller index: dist = sqrtf(d2), idx = i if d2 <= r2 (inclusive), else dist = +inf,
 *                       idx = -1.  max_dist = +inf gives the exact unbounded answer.  Where a query qualifies, dist and idx
 *                       are the bits ncw_nn_query writes when it resolves the query in its shells (the same d2 expression).
 *                       A query with a NaN coordinate gets +inf / -1 without a walk; one with an infinite coordinate has
 *                       d2 = +inf to every point: +inf / 0 when max_dist = +inf, else +inf / -1.
 *                       The walk: fine shells 0..2 as ncw_nn_query, then Chebyshev shells of coarse blocks around the
 *                       query's block.  A block or a cell is skipped when sum_a max(0, gap_a - margin)^2 > min(best d2, r2)
 *                       (strict), gap_a = the distance along axis a from the query to the box of the block / cell; faces on
 *                       the grid boundary give no gap, because points outside the grid box are clamped into the boundary
 *                       cells.  An empty block costs one lookup.  The walk ends when (b - margin) > 0 and
 *                       (b - margin)^2 > min(best d2, r2), b = distance to the faces of the visited blocks that are not on
 *                       the grid boundary, or when the blocks cover the grid.  No atomics: dist / idx are a function of the
 *                       inputs only, bitwise reproducible and the same for any split of the queries into launches.
 *                       NCW_E_BADARG without a launch for a NULL pointer, a bad grid, B not a power of two in [1, 65536],
 *                       margin < 0 or NaN, max_dist <= 0 or NaN; 0 without a launch for n <= 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwNnGrid {
    float lo[3];
    float h, inv_h;
    int32_t dim[3];
} NcwNnGrid;

int ncw_nn_cell_keys(const float* pts, int64_t n, const NcwNnGrid* grid, int32_t* keys, void* stream);
int ncw_nn_cell_ranges(const float* pts, const int32_t* sorted_keys, const int64_t* order, int64_t m, int32_t* cell_range,
                       float* pts_sorted, void* stream);
int ncw_nn_query(const float* pts_sorted, const int32_t* cell_range, const float* q, const int64_t* q_order, int64_t n,
                 const NcwNnGrid* grid, int max_shell, float margin, float* dist, int64_t* idx, int32_t* escaped,
                 int32_t* n_escaped, void* stream);
int ncw_nn_brute(const float* pts_sorted, int64_t m, const float* q, const int32_t* escaped, int64_t n_esc, uint64_t* scratch,
                 float* dist, int64_t* idx, void* stream);
int ncw_nn_coarse(const int32_t* cell_range, const NcwNnGrid* grid, int B, int32_t* coarse, void* stream);
int ncw_nn_query_within(const float* pts_sorted, const int32_t* cell_range, const int32_t* coarse, int B, const float* q,
                        const int64_t* q_order, int64_t n, const NcwNnGrid* grid, float margin, float max_dist, float* dist,
                        int64_t* idx, void* stream);


/* ------------------------------------------------------------------------------------------
 * Exact k nearest neighbours on the grid above, and the PCA of a neighbour list (cloud normals, statistical outlier removal,
 * normal consistency of the mesh evaluation).  The file is built without a * b + c -> fma contraction: d2 = dx*dx + dy*dy +
 * dz*dz with dx = P[i].x - q.x rounds every operation, and so does every float64 operation of ncw_knn_pca.
 *   ncw_knn_query: the tables of a built grid (pts_sorted, cell_range, the coarse level of ncw_nn_coarse and its B), the
 *                  queries q [n,3] f32 and q_order as ncw_nn_query_within.  With r2 = max_dist * max_dist (one float32 product,
 *                  formed by this entry) the admitted set of query j is {(d2(q_j, P[i]), i) : d2 <= r2 (inclusive), i !=
 *                  exclude[j]}; row j gets its k smallest elements under the LEXICOGRAPHIC order (d2, i) -- a tie on d2 goes to the
 *                  smaller index, as in the 1-NN kernels -- in ascending order: idx [n,k] int32, dist [n,k] f32 = sqrtf(d2),
 *                  count [n] int32 = the number of entries; ranks beyond count hold -1 / +inf.  max_dist = +inf: no bound.
 *                  exclude [n] int32 or NULL: an index into P, or -1; that index alone is never reported for query j (a cloud
 *                  querying itself); a duplicate of that point at d = 0 stays.  A query with a NaN or infinite coordinate
 *                  gets count = 0.  1 <= k <= 32; fewer than k admitted points give a short row.
 *                  The walk is ncw_nn_query_within's with min(best d2, r2) replaced by min(kth, r2), kth = the current k-th best
 *                  d2 (+inf while the list is short), every comparison strict as there; each cell is scanned at most once (the
 *                  coarse phase skips the fine cells already walked), so no index repeats in a row.  One launch, no escape
 *                  list, no brute-force pass, no atomics: the outputs are a function of the inputs only, bitwise reproducible
 *                  and the same for any split of the queries into launches.  The candidate list is k x wg (d2, index) pairs
 *                  of LDS; wg = the workgroup size, 64, 128 or 256 (0 = the default, 64).  work [n,2] int32 or NULL: per
 *                  query the distance evaluations and the list insertions (measurement only).
 *                  NCW_E_BADARG without a launch for a NULL pointer (exclude and work excepted), a bad grid, B not a power of two
 *                  in [1, 65536], margin < 0 or NaN, max_dist <= 0 or NaN, k outside [1, 32], another wg; 0 without a
 *                  launch for n <= 0.
 *   ncw_knn_pca  : per point j of pts [n,3] f32 its members: the point itself first when with_query, then
 *                  ref[idx[j, r]] [m,3] f32 for r < count[j] in list order (a list ends at an index outside [0, m)).  In
 *                  float64, every operation rounded once: the mean (sum in member order, / n_j), the six covariance sums of
 *                  (a - mean_a)(b - mean_b) in member order, / n_j; cyclic Jacobi, 8 sweeps of the rotations (0,1), (0,2),
 *                  (1,2), a rotation skipped where its off-diagonal is exactly 0 (theta = (aqq - app) / (2 apq), t = sign(theta)
 *                  / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c); eigenvalues sorted ascending by the
 *                  compare-swaps (0,1), (1,2), (0,1).  eig [n,3] f64 ascending; curvature [n] f32 = l0 / (l0 + l1 + l2), 0
 *                  when the sum is 0; valid [n] uint8 = n_j >= 3 and l1 > 1e-10 l2 (collinear or coincident members have
 *                  no normal); normal [n,3] f32 = the eigenvector of l0 divided by its length, 0 where invalid.  Sign: with
 *                  toward (a HOST pointer to 3 floats, read by this entry; NULL = none) flipped so that n . (toward - p) >= 0 in
 *                  float64; otherwise so that its component of largest magnitude (the first such on ties) is positive.
 *                  n_j = 0 gives zeros.  NCW_E_BADARG for a NULL pointer (toward excepted) or k outside [1, 32].
 * ---------------------------------------------------------------------------------------- */
int ncw_knn_query(const float* pts_sorted, const int32_t* cell_range, const int32_t* coarse, int B, const float* q,
                  const int64_t* q_order, const int32_t* exclude, int64_t n, const NcwNnGrid* grid, float margin, float max_dist,
                  int k, int wg, int32_t* idx, float* dist, int32_t* count, int32_t* work, void* stream);
int ncw_knn_pca(const float* pts, const float* ref, int64_t m, const int32_t* idx, const int32_t* count, int64_t n, int k,
                int with_query, const float* toward, float* normal, double* eig, float* curvature, uint8_t* valid, void* stream);


/* ------------------------------------------------------------------------------------------
 * Implicit-moving-least-squares (IMLS) values of an oriented cloud on a sparse lattice: an all-within-R gather over the grid
 * above (csrc/ncw_imls.hip; cloudmesh.py meshes a cloud with it).  The file is built without a * b + c -> fma contraction: every
 * operation named below rounds once.
 *   ncw_imls_values: the tables of a built grid -- pts_sorted [m][4] f32 (x, y, z, index bits) and cell_range -- the grid and its
 *                  margin; nrm_sorted [m][4] f32: the normal of pts_sorted[i] in (x, y, z) of row i (the caller gathers them
 *                  through the index in pts_sorted.w; .w is not read); blocks [nb][3] int32: coordinates of 4 x 4 x 4 blocks of
 *                  lattice points; the lattice lat_lo[3], voxel, side[3] (lat_lo and side are HOST pointers, read by this
 *                  entry); radius.  Row b * 64 + ((a * 4 + c) * 4 + e) of value [nb*64] f32, count [nb*64] int32 and d2min
 *                  [nb*64] f32 belongs to the lattice point (i_x, i_y, i_z) = (4 bx + a, 4 by + c, 4 bz + e).
 *                  x_a = lat_lo_a + float(i_a) * voxel in float32; r2 = radius * radius (one float32 product, formed by this
 *                  entry); inv_r2 = 1.0 / double(r2).  The admitted set of a lattice point: every i in [0, m), over ALL of P in
 *                  ascending pts_sorted order, with d2 <= r2 (inclusive), d2 = dx*dx + dy*dy + dz*dz in float32 summed left to
 *                  right, dx = P[i].x - x.x (the expression of the 1-NN kernels).  In that order, in float64:
 *                  t = 1 - double(d2) * inv_r2; w = (t * t) * (t * t); g = -((dx * nx + dy * ny) + dz * nz); S += w * g; W += w.
 *                  count = the number admitted; d2min = the smallest admitted d2, +inf when count = 0; value = float(S / W)
 *                  when count > 0 and W > 0, else NaN (a lone point exactly at d2 == r2 has w = 0: NaN).  A lattice index
 *                  outside [0, side) (a negative block coordinate included) writes NaN / 0 / +inf.  A point of P with a
 *                  non-finite coordinate is never admitted.
 *                  One wave per block: it walks the cells of its block's box grown by radius (1 + 2^-20) + margin, clamped to
 *                  the grid (the boundary cells hold the clamped outliers; the kernel's header argues that this is a superset
 *                  of what d2 <= r2 can admit), in cell order, and stages their points through LDS; every lane tests every
 *                  staged point.  No atomics, no transcendental function, no square root: the outputs are a function of the
 *                  inputs only, bitwise reproducible and the same for any order or split of `blocks` into launches.
 *                  work [nb] int32 or NULL: the points staged per block (measurement only).
 *                  NCW_E_BADARG without a launch for a NULL pointer (work excepted), a bad grid, m outside [1, 2^31), voxel <= 0,
 *                  infinite or NaN, radius <= 0 or NaN or with r2 not a finite normal number, margin < 0, infinite or NaN, a side
 *                  outside 1 .. 16384, nb >= 2^25; 0 without a launch for nb <= 0.
 * ---------------------------------------------------------------------------------------- */
int ncw_imls_values(const float* pts_sorted, const float* nrm_sorted, const int32_t* cell_range, int64_t m, const NcwNnGrid* grid,
                    float margin, const int32_t* blocks, int64_t nb, const float* lat_lo, float voxel, const int32_t* side,
                    float radius, float* value, int32_t* count, float* d2min, int32_t* work, void* stream);


/* ------------------------------------------------------------------------------------------
 * Triangle depth rasterizer of the reprojection visibility filter: replaces the pyrender depth render of
 * utils/pyrender_renderer.py:16-24 (utils/reproj_filter.py:208), the back-projection `reproject` of
 * utils/reproj_filter.py:133-152 and the per-pixel open3d KD-tree marking loop of :229-232 (with ncw_nn_*).
 * One view: camera = view[:, :3] v + view[:, 3] (row-major 3x4, OpenCV axes: x right, y down, looking along +z); pixel
 * (r, c) samples the image point (c + 0.5, r + 0.5) of u = fx x / z + cx, v = fy y / z + cy; linear depth z.  Faces with
 * every vertex in front of znear or beyond zfar are dropped, faces crossing znear are clipped to it (OpenGL's clip), samples
 * beyond zfar are dropped.  cull = 1 drops back faces (signed area > 0 in pixel coordinates), 0 draws both sides; zero-area
 * triangles are dropped.  A sample is covered when all three edge functions are >= 0 (antisymmetric on shared edges: no
 * holes).  Depth is perspective-correct; the z-buffer zbuf[height * width] uint64 (filled with 0xff.. by the caller) is a
 * 64-bit atomicMin of (float bits of z << 32 | face): nearest first, equal depth to the smaller face, order-independent.
 *   ncw_raster_small      : every face; sub-triangles whose pixel box holds at most small_max samples are rasterized by
 *                           their lane, the others appended as (2 face + sub) to large[] (capacity 2 n_faces, count in
 *                           *n_large, zeroed by the caller).  n_faces < 2^30.
 *   ncw_raster_large      : the large list (min(*n_large, max_large) entries), one workgroup per entry.
 *   ncw_raster_resolve    : depth[n_pix] f32 (0 = empty), face[n_pix] int32 (-1 = empty; NULL = not written).
 *   ncw_raster_backproject: for the n listed pixels pix[] (linear r * width + c), pts[n][3] = M[:, :3] (c d, r d, d) + M[:, 3]
 *                           with d = depth[pix] and M row-major 3x4 on the host (pose K^-1 | pose translation): the
 *                           reference's INTEGER pixel coordinates.
 *   ncw_raster_mark       : flags[idx[i]] = 1 (uint8[m]) for every i < n with dist[i] < thr.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwRasterView {
    float view[12];
    float fx, fy, cx, cy;
    float znear, zfar;
    int32_t height, width;
    int32_t cull;
    int32_t small_max;
} NcwRasterView;

int ncw_raster_small(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const NcwRasterView* view,
                     uint64_t* zbuf, int32_t* large, int32_t* n_large, void* stream);
int ncw_raster_large(const float* verts, int64_t n_verts, const int32_t* faces, const NcwRasterView* view, const int32_t* large,
                     const int32_t* n_large, int64_t max_large, uint64_t* zbuf, void* stream);
int ncw_raster_resolve(const uint64_t* zbuf, int64_t n_pix, float* depth, int32_t* face, void* stream);
int ncw_raster_backproject(const float* depth, const int64_t* pix, int64_t n, int32_t width, const float* M, float* pts,
                           void* stream);
int ncw_raster_mark(const float* dist, const int64_t* idx, int64_t n, float thr, int64_t m, uint8_t* flags, void* stream);


/* ------------------------------------------------------------------------------------------
 * Camera views (csrc/ncw_view.hip): what surrounds the forward-only render of one whole view in the reference's validation step
 * (lightning_modules/neuconw_system.py:404-464, 533-546) -- ray generation, assembly of the chunk outputs into image planes, the
 * depth colour map and the image metrics -- on the device, without a host round trip per chunk.  Every reduction is two-stage
 * and fixed-order (no float atomics): bitwise reproducible run to run.  Images are f32; pixels are row-major.
 *   ncw_view_rays     : datasets/ray_utils.py:18-52 (get_ray_directions + get_rays) and datasets/phototourism.py:769-782 for the
 *                       pixels [p0, p0 + n) of the view: rays[n][8] = o, d, near, far.  Pixel (row j, column i), INTEGER
 *                       coordinates (no + 0.5): dir = ((i - cx) / fx, -(j - cy) / fy, -1), d = c2w[:, :3] dir normalised,
 *                       o = c2w[:, 3].  cam is a HOST struct (c2w row-major 3x4, "right up back" axes).  rays must be 16-byte
 *                       aligned (rows are written as two 16-byte stores); returns -1 otherwise, or for a range outside the view.
 *   ncw_view_store    : neuconw_system.py:440-460: one chunk's color [n,3] / depth [n] / compositor normals [n,3]
 *                       (NcwCompositeOut.normals = sum_s gradients weights) to pixel offset p0 of the planar color_img [3,n_pix],
 *                       depth_img [n_pix], normal_img [3,n_pix]; the normal plane holds v / |v| / 2 + 0.5 (0 / 0 stays NaN, as
 *                       there).  Any of the three inputs may be NULL (not written).
 *   ncw_image_minmax  : utils/visualization.py:18-20: minmax[2] (device) = min, max of nan_to_num(x[n]) (NaN -> 0, +-inf ->
 *                       +-FLT_MAX), n >= 1.  scratch: ncw_image_reduce_scratch_bytes() bytes.
 *   ncw_depth_colormap: utils/visualization.py:21-24: index = uint8(255 * ((x - mi) / (ma - mi + 1e-8))) in f32 with IEEE
 *                       division and truncation (NaN from inf / inf -> 0), looked up in lut [256][3] uint8 (RGB);
 *                       out_f32 [3,n] = value / 255 (torchvision ToTensor), out_u8 [3,n], out_index [n]: each may be NULL.
 *   ncw_image_sqerr   : metrics.py:5-14: sum_out[1] f32 = sum of (pred - gt)^2 and count_out[1] int64 = number of elements over
 *                       n pixels of 3 channels ([n,3], or planar [3,n] with planar = 1), restricted to the pixels with
 *                       mask[i] != 0 when mask (uint8 [n]) is not NULL.  mse = sum / count, psnr = -10 log10(mse).
 *   ncw_image_ssim    : metrics.py:16-21 over kornia's ssim(pred, gt, window, 'mean'): separable Gaussian window (sigma 1.5,
 *                       window in {3, 5, 7, 9, 11}), reflect padding of (window - 1) / 2, moments mu_x, mu_y, E[x^2], E[y^2],
 *                       E[xy] per channel, C1 = 0.01^2, C2 = 0.03^2, map = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 +
 *                       C1)(s_x^2 + s_y^2 + C2)); ssim_out[1] = mean over pixels and channels of clamp(map, -1, 1), which
 *                       equals the reference's 1 - 2 mean(clamp((1 - map) / 2, 0, 1)).  pred / gt planar [channels, height,
 *                       width]; scratch: ncw_image_ssim_scratch_floats(channels, height, width) floats.  Returns -2 when
 *                       height or width <= (window - 1) / 2 (reflect padding is undefined there), -1 for a bad window.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwViewCamera {
    float fx, fy, cx, cy;
    float c2w[12];
    int32_t width, height;
    float near, far;
} NcwViewCamera;

int ncw_view_rays(const NcwViewCamera* cam, int64_t p0, int64_t n, float* rays, void* stream);
int ncw_view_store(const float* color, const float* depth, const float* normals, int64_t p0, int64_t n, int64_t n_pix,
                   float* color_img, float* depth_img, float* normal_img, void* stream);
int64_t ncw_image_reduce_scratch_bytes(void);
int ncw_image_minmax(const float* x, int64_t n, void* scratch, float* minmax, void* stream);
int ncw_depth_colormap(const float* depth, int64_t n, const float* minmax, const uint8_t* lut, float* out_f32, uint8_t* out_u8,
                       uint8_t* out_index, void* stream);
int ncw_image_sqerr(const float* pred, const float* gt, const uint8_t* mask, int64_t n, int planar, void* scratch, float* sum_out,
                    int64_t* count_out, void* stream);
int64_t ncw_image_ssim_scratch_floats(int channels, int height, int width);
int ncw_image_ssim(const float* pred, const float* gt, int channels, int height, int width, int window, float* scratch,
                   float* ssim_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Surface views by sphere tracing (csrc/ncw_trace.hip; not in the reference): the per-ray march that finds the first point with
 * |sdf| <= eps along o + t d, t in [near, far], |d| = 1.  The SDF itself is evaluated BETWEEN these launches by the value path
 * (ncw_sdf_infer) on the points they emit.  Everything is float32 with every product, quotient and sum rounded once (no FMA
 * contraction, IEEE division), so that a numpy float32 restatement reproduces it bit for bit (tests/_trace_ref.py).
 *
 *   state = ACTIVE if far > near else MISS (0 evaluations);  t = near;  bracketed = 0
 *   each evaluation k = 1, 2, ...:  p = o + t d (mul, then add, per component);  s = sdf(p);  iters += 1
 *     s not finite -> STALLED;   |s| <= eps -> HIT (depth t);   s > 0 -> t_lo = t, s_lo = s;
 *     s < 0: k == 1 -> INSIDE (the interval starts below the surface);  else t_hi = t, s_hi = s, bracketed = max(bracketed, 1)
 *     not bracketed:  t' = t + step s;  t' > far -> MISS;  else t = t'
 *     bracketed:      w = t_hi - t_lo;  odd count: t = t_lo + (s_lo w) / (s_lo - s_hi) (false position);
 *                     even count: t = t_lo + 0.5 w (bisection);  bracketed += 1
 *     iters == max_iter and still ACTIVE -> STALLED
 *
 * The bracket keeps the walk convergent where |grad sdf| > 1 (plain t += s stalls or oscillates there).  It cannot find a surface
 * the walk jumped over entirely (both crossings inside one step: possible only where |grad sdf| step > 1); step < 1 is for that.
 *
 * rec [R][NCW_TRACE_REC_WORDS] 32-bit words per ray: t, t_lo, s_lo, t_hi, s_hi (f32) and one packed word: bits 0-3 the state
 * (0 ACTIVE, NCW_TRACE_*), bits 4-17 the bracket count, bits 18-31 iters (hence max_iter <= NCW_TRACE_MAX_ITER).
 * An ACTIVE LIST is ray indices int32 [m], ASCENDING, with its length in a DEVICE int32 `count`; its points [m][3] are o + t d of
 * the listed rays in list order.  Lists are compacted order-preserving by a two-stage fixed-order scan (per-workgroup counts in
 * `scratch`, ncw_trace_scratch_bytes(R) bytes, at least 4-byte aligned): no atomics of any kind, bitwise reproducible.
 *
 *   ncw_trace_begin : initialises rec for R rays (rays_o / rays_d [R][3], near / far [R]) and writes the first active list
 *                     (the rays with far > near), *count and its points.
 *   ncw_trace_step  : consumes sdf [m] of the list (active_in, *count_in): updates rec by one evaluation of the recurrence above
 *                     and writes the list of the rays still ACTIVE (active_out, *count_out) and their next points.  m_bound is an
 *                     UPPER BOUND of *count_in known to the host (the grid size); the kernels read the count itself from the
 *                     device, so the host may read it back as rarely as it likes.  Entries of sdf / points past the count are
 *                     ignored / left alone.  active_out / count_out must not alias active_in / count_in.
 *   ncw_trace_finish: unpacks rec into t [R] (HIT: the hit depth; INSIDE: near; otherwise the last depth of the recurrence),
 *                     state [R] uint8, iters [R] int32 and points [R][3] = o + t d; each output may be NULL.
 *   ncw_trace_store : one chunk of n pixels at offset p0 into the planes of a view of n_pix pixels (layout of ncw_view_store):
 *                     depth_img = t at a HIT and 0 elsewhere, state_img uint8, iters_img int32; colour and normal planes get
 *                     background[3] (HOST floats) and 0 at every pixel, then rgb [n_hit][3] and g / |g| / 2 + 0.5 of grad [n_hit][3]
 *                     at the pixels p0 + hit_idx[j] (int64, ascending, each a HIT of this chunk).  n_hit == 0: no second launch.
 *
 * All return NCW_E_BADARG without a launch for a NULL or misaligned (4 bytes; hit_idx 8) pointer, R / m_bound / n outside
 * [0, 2^31 - 1], m_bound > R, eps <= 0, step outside (0, 1], max_iter outside [1, NCW_TRACE_MAX_ITER] (NaNs included) or a
 * range outside the view; 0 without a launch for R == 0 (begin: *count is then NOT written), m_bound == 0 and n == 0.
 * ---------------------------------------------------------------------------------------- */
#define NCW_TRACE_HIT 1
#define NCW_TRACE_MISS 2
#define NCW_TRACE_INSIDE 3
#define NCW_TRACE_STALLED 4
#define NCW_TRACE_REC_WORDS 6
#define NCW_TRACE_MAX_ITER 16383
int64_t ncw_trace_scratch_bytes(int64_t R);
int ncw_trace_begin(const float* rays_o, const float* rays_d, const float* near, const float* far, int64_t R, float* rec,
                    int32_t* active, int32_t* count, float* points, void* scratch, void* stream);
int ncw_trace_step(const float* sdf, const int32_t* active_in, const int32_t* count_in, int64_t m_bound, const float* rays_o,
                   const float* rays_d, const float* far, int64_t R, float eps, float step, int max_iter, float* rec,
                   int32_t* active_out, int32_t* count_out, float* points, void* scratch, void* stream);
int ncw_trace_finish(const float* rec, const float* rays_o, const float* rays_d, int64_t R, float* t, uint8_t* state,
                     int32_t* iters, float* points, void* stream);
int ncw_trace_store(const float* t, const uint8_t* state, const int32_t* iters, const int64_t* hit_idx, const float* rgb,
                    const float* grad, int64_t n_hit, const float* background_host, int64_t p0, int64_t n, int64_t n_pix,
                    float* color_img, float* depth_img, float* normal_img, uint8_t* state_img, int32_t* iters_img, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray cache (csrc/ncw_cache.hip): the training rows of ONE image as the reference's dataset builds them for
 * tools/prepare_data/prepare_data_cache.py (datasets/phototourism.py:150-209, 557-657), without its host round trips.
 *   ncw_sfm_depth_splat : get_colmap_depth (:150-209) without the dir_norm factor (ncw_cache_rows applies it): the n SfM
 *                         key-points of the image -- xyz [n,3] f32 world positions, err [n] f32 reprojection errors, px [n,2]
 *                         int32 (col, row), already rounded -- as planes depth_z [h*w] (camera-space z = row 2 of the HOST
 *                         world -> camera matrix w2c_host[12] applied to the point; K's last row is (0, 0, 1), so the
 *                         reference's `intrinsic @ extrinsic` leaves that row as it is; negative z is written as it is) and
 *                         weight [h*w] = 2 exp(-(err / err_mean)^2); zero where no key-point lands.  Key-points outside
 *                         [0,w) x [0,h) are ignored.  Where several land on one pixel THE LARGEST INDEX WINS (file order, what
 *                         numpy / torch-CPU assignment does; the reference's CUDA assignment is unordered): pass 1 is an int32
 *                         atomicMax into `winner` [h*w] (scratch), pass 2 lets the winner write.  No float atomics: bitwise
 *                         reproducible.  The three planes are filled by the entry point; n == 0 launches no kernel.
 *   ncw_cache_rows      : :557-657 for the pixels [p0, p0 + n) of the view (row-major), one thread per pixel:
 *                         rows [n][ncols] = o(3) d(3) near far ts [label] depth weight 0 (ncols 13 with a label map, 12 with
 *                         label == NULL: the layout ncw_batch_assemble reads; the reference's code concatenates these columns
 *                         WITHOUT the last one although its comment and its reader's [10:13] say 13), rgbs [n][3] = float(u8) / 255.f of image [h,w,3] uint8, keep [n] uint8.
 *                         o, d: ncw_view_rays' arithmetic.  depth = depth_z[p] |((col - cx) / fx, (row - cy) / fy, 1)|.
 *                         label: nearest sample of the uint8 map [label_h, label_w] at (floor(row label_h / h), floor(col
 *                         label_w / w)), clamped (stands in for cv2.resize INTER_NEAREST; unpinned against cv2).
 *                         hit / range: the SfM octrees of gen_octree_from_sfm(expand=1, radius=1) / (expand=2, radius=1.5)
 *                         (HOST structs; either NULL = use_voxel False: keep = 1 and near / far are the camera's).  keep = 1
 *                         iff ncw_ray_voxel_near_far's near of the hit octree is > 0; where keep, near / far become the range
 *                         octree's near and far + voxel_size, or 0 / 0 where it misses.  Rows of dropped pixels are written
 *                         too (camera near / far).  rows and rgbs must be 16-byte aligned (workgroups write 16-byte stores).
 * Both return NCW_E_BADARG for NULL / misaligned pointers or a range outside the view, 0 without a launch for n == 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwCacheOctree {
    float origin[3];
    float scale;
    int32_t level;
    int32_t _pad;
    const uint32_t* occ;
    const uint32_t* brick;
} NcwCacheOctree;

int ncw_sfm_depth_splat(const float* xyz, const float* err, const int32_t* px, int64_t n, double err_mean, const float* w2c_host,
                        int width, int height, int32_t* winner, float* depth_z, float* weight, void* stream);
int ncw_cache_rows(const NcwViewCamera* cam, const uint8_t* image, const uint8_t* label, int label_h, int label_w,
                   const float* depth_z, const float* weight, int image_id, float voxel_size, const NcwCacheOctree* hit,
                   const NcwCacheOctree* range, int64_t p0, int64_t n, int ncols, float* rows, float* rgbs, uint8_t* keep,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray source (csrc/ncw_source.hip): a training batch rebuilt from the scene itself instead of gathered from cached rows --
 * what ncw_cache_rows (datasets/phototourism.py:557-657) followed by ncw_batch_assemble (datasets/phototourism.py:709-726 +
 * the black-list test of neuconw_system.py:345-349) returns for the same rays, bit for bit, from 8 bytes per kept ray.
 *   recs [n_rows]        : NcwSourceRec, one per kept ray, grouped by image in table order:
 *                            pix   bits 0..30 = row-major pixel index in its image (row = pix / width, col = pix % width);
 *                                  bit 31 set = the pixel carries an SfM key-point (an entry of the key-point table);
 *                            r, g, b = the image's uint8 pixel (rgbs = float(u8) / 255.f, as ncw_cache_rows writes it);
 *                            label = the label-map sample ncw_cache_rows put in the row; 0 when the source has no label maps.
 *   images [n_img]       : NcwSourceImage = the view (with the camera's own near / far) and ts = the COLMAP image id.
 *   row_start [n_img + 1]: int64, records [row_start[k], row_start[k + 1]) belong to image k; an image without a record repeats
 *                          the previous start.  row_start[0] = 0, row_start[n_img] = n_rows.
 *   kp_start [n_img + 1] : int64, the same for the key-point table: kp_pix (int32, ascending within an image), kp_depth (f32, the
 *                          along-ray depth as ncw_cache_rows writes it), kp_weight (f32).  Only records with bit 31 search it (a
 *                          binary search over the image's segment); a record whose pixel is not found gets depth = weight = 0.
 *                          The three arrays may be NULL when no record has bit 31 set.
 *   range, voxel_size    : the range octree (HOST struct) or NULL.  A record exists only for a pixel the hit octree kept, so only
 *                          this one is walked: near = rn, far = rn > 0 ? rf + voxel_size : rf.  NULL: the camera's near / far.
 *   idx [B]              : int64 record indices, clamped to [0, n_rows) as ncw_batch_assemble clamps; NULL = the identity.
 *   outputs              : ncw_batch_assemble's -- rays [B][11] = o(3) d(3) near far depth weight 0, ts [B] int64, label [B]
 *                          int64 or NULL, rgbs [B][3], keep [B] uint8 or NULL (0 where with_semantics and label is one of the
 *                          n_ids <= 4 HOST mask_ids).  with_semantics == 0: label = 0 and keep = 1.
 * One lane per batch row, one launch per batch; o, d, near, far come from the device functions ncw_cache_rows uses
 * (csrc/ncw_rowmath.h).  No atomics: bitwise reproducible and independent of how a set of indices is split into launches.
 * rays and rgbs must be 16-byte aligned (workgroups write 16-byte stores).  Returns NCW_E_BADARG for NULL / misaligned pointers,
 * n_rows <= 0, n_img <= 0, n_ids outside 0..4 or a bad octree; 0 without a launch for B <= 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwSourceRec {
    uint32_t pix;
    uint8_t r, g, b, label;
} NcwSourceRec;

typedef struct NcwSourceImage {
    NcwViewCamera cam;
    int32_t ts;
    int32_t _pad;
} NcwSourceImage;

int ncw_source_batch(const NcwSourceRec* recs, int64_t n_rows, const NcwSourceImage* images, const int64_t* row_start,
                     const int64_t* kp_start, int n_img, const int32_t* kp_pix, const float* kp_depth, const float* kp_weight,
                     const NcwCacheOctree* range, float voxel_size, const int64_t* idx, int64_t B, int with_semantics, float* rays,
                     int64_t* ts, int64_t* label, float* rgbs, const int* mask_ids, int n_ids, uint8_t* keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voxel first-hit views (csrc/ncw_voxview.hip): the point-cloud source of the reprojection filter.  The reference voxelises
 * the source cloud over the evaluation box (utils/kaolin_renderer.py:16-17: gen_octree(..., expand=0, in_sfm=False)), traces
 * every pixel of every training view to the first occupied voxel (:110-141) and keeps the target points whose voxel some
 * view saw (utils/reproj_filter.py:195-196, 224-225, 234-240).  UNPINNED against kaolin (its source is not in the reference
 * tree): as for ncw_ray_voxel_trace the contract followed is its documented one, pinned to the float64 slab oracle.
 *   ncw_voxel_view_seen   : replaces kaolin_renderer.py:33-51 (gen_rays) + :110-141 (__call__) + generate_voxel.py:311-439
 *                           (get_near_far, return_pts) + reproj_filter.py:224-225 for ONE view, pixels [p0, p0 + n) row-major,
 *                           one lane per pixel.  view: HOST struct; pose = row-major 3x3 camera -> world part of
 *                           inv(E inv(sfm2gt)) (OpenCV axes, scale included), o_norm = (camera centre + 1e-7 - box centre) /
 *                           scale computed by the host in float64 (generate_voxel.py:333, :345).  Ray of pixel (row j, col i):
 *                           dir = pose ((i - cx) / fx, (j - cy) / fy, 1), dir_norm = |dir|, d = dir / dir_norm + 1e-7 per
 *                           component (:332); grid coordinates and depths as ncw_ray_voxel_near_far's.  The walk STOPS at the
 *                           first occupied voxel in depth order; the ray is valid iff that voxel's entry depth is > 1e-4
 *                           (:397-400: a camera inside an occupied voxel sees nothing along that ray).  grid: HOST struct
 *                           (origin is not read; scale turns depths into the units of the box).  A valid ray sets its
 *                           voxel's bit in seen (same layout and size as grid->occ; atomicOr, issued only when a plain load
 *                           finds the bit clear: the grid only gains bits, so the result is order-independent and bitwise
 *                           reproducible), voxel[p - p0] = (x G + y) G + z, depth[p - p0] = near scale / dir_norm + 0.02
 *                           (kaolin_renderer.py:127, 141: camera-space z).  Any other ray sets nothing, voxel = -1, depth = 0
 *                           (the reference's pid = -1 wraps round and marks an unrelated voxel, and its depth is 0.02: neither
 *                           is reproduced).  seen is NOT cleared: views accumulate.  depth / voxel: optional planes [n]
 *                           (NULL = not written).
 *   ncw_voxel_points_seen : replaces kaolin_renderer.py:53-107 (get_index over vertex_table) for any target:
 *                           flags[i] (uint8) = the bit in seen of the voxel of normalised point i (f32 [n,3]), the voxel
 *                           computed with ncw_voxel_build's arithmetic ((p + 1) (0.5f G), truncated); 0 for a point outside
 *                           the cube or NaN (:102, voxel_id = -10).
 * Both return NCW_E_BADARG for NULL grid / seen pointers, a level outside 3..10 or a range outside the view; 0 without a
 * launch for n == 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwVoxelView {
    float fx, fy, cx, cy;
    float pose[9];
    float o_norm[3];
    int32_t width, height;
} NcwVoxelView;

int ncw_voxel_view_seen(const NcwVoxelView* view, const NcwCacheOctree* grid, int64_t p0, int64_t n, uint32_t* seen,
                        float* depth, int32_t* voxel, void* stream);
int ncw_voxel_points_seen(const float* pts_normalised, int64_t n, int level, const uint32_t* seen, uint8_t* flags,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Area-weighted surface sampling of a triangle mesh (csrc/ncw_surf.hip) for the mesh evaluation: the open3d branch of the
 * reference scores a predicted MESH by 10 |GT| points drawn uniformly by area from the triangles inside the evaluation box
 * (utils/eval_utils.py:20-61: `mesh_pred.crop(bbox_gt)` :39, `sample_points_uniformly` :42) and colours the two clouds by
 * their errors (:116-123, host side: evalmesh.error_colours).  All arithmetic is float64 (GT coordinates are metres far from
 * the origin, triangles are millimetres); no atomics; every output depends on its own index only, so results are bitwise
 * reproducible and a range of samples may be split over any number of launches.
 * UNPINNED against open3d (its source is not at hand): the crop rule -- taken from its documentation: a triangle survives
 * when all three vertices are inside the box, bounds inclusive --, and the random stream (open3d draws from an unseeded
 * Mersenne twister: its samples are not reproducible even in the reference).
 *   ncw_surf_weights : weight[f] = 0.5 |(B - A) x (C - A)| of faces [F,3] int32 over verts [V,3] f64; EXACTLY 0 when a corner
 *                      index is outside [0, n_verts) (such a corner is never read), when the area is not finite, or when
 *                      `box` (HOST double[6]: lo xyz, hi xyz; NULL = no crop) is given and any corner lies outside the
 *                      closed box.
 *   (caller)         : cdf[f] = inclusive prefix sum of weight in f64, non-decreasing (evalmesh.surface_cdf: torch.cumsum).
 *   ncw_surf_pick    : tri[i] = the smallest k with cdf[k] > x[i]; when there is none (x >= cdf[F-1]) the smallest k with
 *                      cdf[k] == cdf[F-1] (the last triangle of positive weight).  NaN or negative x counts as 0.  A triangle
 *                      of weight 0 (cdf[k] == cdf[k-1], or cdf[0] == 0) is therefore never returned.  n_faces >= 1.
 *   ncw_surf_sample  : samples i = i0 .. i0 + n - 1 of n_total, one lane each.  (w0, w1, w2, w3) = Philox4x32-10 of counter
 *                      (lo32(i), hi32(i), 0, 0) under key (lo32(seed), hi32(seed));  xi = (((u64)w0 << 32 | w1) >> 11) 2^-53,
 *                      r1 = (w2 + 0.5) 2^-32, r2 = (w3 + 0.5) 2^-32;  mode 0 (independent draws, the reference's
 *                      distribution): u = xi;  mode 1 (stratified): u = (i + xi) / n_total;  k = pick(u cdf[F-1]) with
 *                      ncw_surf_pick's search;  s = sqrt(r1), pts[i - i0] = (1 - s) A + s (1 - r2) B + s r2 C (open3d's
 *                      formula; products and sums rounded one by one, no FMA).  tri [n] int32 (k) and urr [n,3] f64
 *                      (u, r1, r2) are optional (NULL = not written).  The caller guarantees that every face of positive
 *                      weight has its corners inside verts (ncw_surf_weights' zeros do).  When cdf[F-1] is not > 0 there is
 *                      nothing to draw from: no face is read, pts are NaN and tri is -1.
 * All return NCW_E_BADARG for NULL pointers, n_faces outside [1, 2^31) (pick / sample), a bad mode, or (mode 1) a range
 * outside [0, n_total); 0 without a launch for an empty range.
 * ---------------------------------------------------------------------------------------- */
int ncw_surf_weights(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* box,
                     double* weight, void* stream);
int ncw_surf_pick(const double* cdf, int64_t n_faces, const double* x, int64_t n, int32_t* tri, void* stream);
int ncw_surf_sample(const double* verts, const int32_t* faces, const double* cdf, int64_t n_faces, uint64_t seed, int64_t i0,
                    int64_t n, int64_t n_total, int mode, double* pts, int32_t* tri, double* urr, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact point-to-triangle-mesh distances (csrc/ncw_ptm.hip): the recall side of the mesh evaluation measured to the
 * predicted SURFACE, not to samples of it (what trimesh `proximity`, kaolin `point_to_mesh_distance` or open3d
 * `RaycastingScene` answer; no parity with any of them is pinned: none is at hand).  The uniform-grid shell search of
 * ncw_nn_*, carried from points to triangles.  All arithmetic is float64 on coordinates recentred in float64; products and
 * sums are rounded one by one (no FMA), so tests/_ptm_ref.py restates the same arithmetic.
 * DISTANCE CONTRACT.  Query P, triangle (A, B, C):
 *   face term : n = (B-A)x(C-A), nn = n.n; exists iff nn > 0, nn finite and the three edge functions ((B-A)x(P-A)).n,
 *               ((C-B)x(P-B)).n, ((A-C)x(P-C)).n are all >= 0; d^2 = t^2 / nn with t = n.(P-A); closest = P - (t/nn) n.
 *   segments  : AB, BC, CA, endpoints in CANONICAL order (the lexicographically smaller coordinate triple is U, the other
 *               V; equal endpoints stay): w = V-U, l = w.w, s = l > 0 ? clamp(((P-U).w)/l, 0, 1) : 0; closest c = U if
 *               s <= 0, V if s >= 1, else U + s w; d^2 = |P-c|^2 from the coordinate differences.
 *   triangle  : the minimum of the terms that exist; closest point of the FIRST minimal term in the order face, AB, BC, CA.
 *               Degenerate triangles need no special case (the face term drops out).
 *   mesh      : the minimum over the VALID triangles, ties on equal d^2 to the SMALLER triangle index.  Valid: all three
 *               corner indices in [0, n_verts), all nine coordinates finite and, with a box (HOST double[6]: lo xyz, hi xyz, in
 *               the coordinates of verts; NULL = none), all three corners inside the closed box (ncw_surf_weights' rule).
 *               An invalid triangle's corners are never read and it is never returned.
 * Canonical endpoints make a shared edge or vertex give bit-identical d^2 from every triangle that owns it.
 * GRID.  Cubic cells of side h over [lo, lo + dim h); cell = clamp(floor((x - lo) inv_h), 0, dim - 1) per axis, linear key
 * (cx dim[1] + cy) dim[2] + cz (x slowest).  A triangle belongs to every cell its axis-aligned box overlaps (cell range
 * clamped into the grid); one whose box covers more than max_cells_per_tri cells stays out of the grid (large list).
 *   ncw_ptm_pack      : tri [F][9] f64 = the recentred corners (A, B, C) minus centre (HOST double[3]) of faces [F,3] int32 over
 *                       verts [V,3] f64; valid [F] uint8.  Invalid rows of tri are zero.
 *   ncw_ptm_count     : count [F] int32 = cells of the triangle's box, or 0 when it is invalid or large;
 *                       large [F] uint8 = 1 for a valid triangle with more than max_cells_per_tri (1 .. 2^30) cells.
 *   (caller)          : cum = inclusive prefix sum of count in int64 (torch.cumsum); n_pairs = cum[F-1] <= 2^31 - 1.
 *   ncw_ptm_emit      : keys [n_pairs] int32 / ids [n_pairs] int32: pair cum[f] - count[f] + k = (k-th cell, f).
 *   (caller)          : stable sort of the pairs by key (torch.sort): sorted_keys, order.
 *   ncw_ptm_ranges    : cell_range [n_cells][2] int32 (ZEROED by the caller) gets [start, end) of every non-empty cell;
 *                       sorted_ids [n_pairs] int32 = ids in cell order.
 *   ncw_ptm_cell_keys : keys [n] int32 of n recentred queries q [n,3] f64.
 *   ncw_ptm_query     : one lane per query in cell order (q_order: stable sort of the query keys).  The large list
 *                       (large_ids [n_large] int32, may be NULL when n_large == 0) is tested first, staged through LDS; then
 *                       Chebyshev shells r = 0, 1, .. around the query's cell, stopping after shell r once
 *                       best d^2 < (b - margin)^2 (b = distance to the faces of the (2r+1)^3 block not on the grid boundary:
 *                       an unvisited triangle's box does not overlap the block, so it lies beyond one of them) or once the
 *                       block covers the grid.  Outputs at the query's ORIGINAL position: dist [n] f64 = sqrt(d^2), idx [n]
 *                       int64, closest [n,3] f64 (NULL = not written).  Queries still open after max_shell shells are
 *                       appended to escaped [n] int32 (their count in *n_escaped, zeroed by the caller) and left unwritten.
 *   ncw_ptm_brute     : the escaped queries against all valid triangles (LDS tiles, triangles split over blocks): a 64-bit
 *                       atomicMin of the bits of d^2 (>= 0: ordered like the value), a second pass with an atomicMin of the
 *                       index among the triangles at that minimum, a finish pass writing the outputs.  scratch:
 *                       uint64 [2 n_esc].  A query that no triangle answers (NaN coordinates) gets dist +inf, idx -1.
 * No float atomics: results are bitwise reproducible, and identical for any split of the queries into launches.
 * All return NCW_E_BADARG for NULL pointers, a bad grid (h, inv_h not > 0, dim < 1, more than 2^30 cells) or counts out of
 * range (n_faces, n_pairs, n_esc > 2^31 - 1, n_verts < 0, max_shell < 0, margin not >= 0); 0 without a launch for an empty range.
 * ---------------------------------------------------------------------------------------- */
typedef struct NcwPtmGrid {
    double lo[3];
    double h, inv_h;
    int32_t dim[3];
} NcwPtmGrid;

int ncw_ptm_pack(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* centre,
                 const double* box, double* tri, uint8_t* valid, void* stream);
int ncw_ptm_count(const double* tri, const uint8_t* valid, int64_t n_faces, const NcwPtmGrid* grid, int64_t max_cells_per_tri,
                  int32_t* count, uint8_t* large, void* stream);
int ncw_ptm_emit(const double* tri, const int32_t* count, const int64_t* cum, int64_t n_faces, const NcwPtmGrid* grid,
                 int64_t n_pairs, int32_t* keys, int32_t* ids, void* stream);
int ncw_ptm_ranges(const int32_t* sorted_keys, const int64_t* order, const int32_t* ids, int64_t n_pairs, int64_t n_cells,
                   int32_t* cell_range, int32_t* sorted_ids, void* stream);
int ncw_ptm_cell_keys(const double* q, int64_t n, const NcwPtmGrid* grid, int32_t* keys, void* stream);
int ncw_ptm_query(const double* tri, int64_t n_faces, const int32_t* cell_range, const int32_t* sorted_ids,
                  const int32_t* large_ids, int64_t n_large, const double* q, const int64_t* q_order, int64_t n,
                  const NcwPtmGrid* grid, int max_shell, double margin, double* dist, int64_t* idx, double* closest,
                  int32_t* escaped, int32_t* n_escaped, void* stream);
int ncw_ptm_brute(const double* tri, const uint8_t* valid, int64_t n_faces, const double* q, int64_t n, const int32_t* escaped,
                  int64_t n_esc, uint64_t* scratch, double* dist, int64_t* idx, double* closest, void* stream);

/* ------------------------------------------------------------------------------------------
 * View selection (csrc/ncw_roi.hip): the region-of-interest test of the split writer, for ALL registered views of a scene in
 * one launch.  The reference runs it per image (tools/prepare_data/dataset_filter_utils.py:160-178: get_ray_directions +
 * get_rays + eight torch ops, after a full decode of the image that is only used for its size); it needs no per-pixel input.
 *   ncw_views_roi : cams_dev [n_views] (DEVICE table; near / far are not read), pix_start_dev [n_views + 1] int64 (DEVICE): the
 *                   exclusive prefix sum of width * height, so that pixel (row, col) of view v is global pixel
 *                   pix_start[v] + row * width + col.  Ray of the pixel: ncw_view_rays' arithmetic (integer pixel
 *                   coordinates, o = c2w[:, 3], d normalised).  In float32, in the reference's order of operations (:171-177),
 *                   with origin_host[3] and radius the scene sphere of config.yaml:
 *                       c = origin - o;  dot = sum(c * d);  p = dot * d;  dist_ray = |c - p|;  dist_cam = |c|
 *                       roi = (radius > dist_cam  or  dot > 0)  and  dist_ray < radius
 *                   count_dev [n_views] uint32 = number of roi pixels of each view (:178 is count / (w h)); the entry point
 *                   clears it on `stream`.  Per wave the 64-bit ballot and its population count, across the waves integer
 *                   adds in LDS, then one integer atomicAdd per workgroup and view it touches (a workgroup's run of pixels
 *                   may straddle views; past eight views per run the adds are per wave): no float atomics, the counts are
 *                   bitwise reproducible.  mask_dev: NULL, or
 *                   [pix_start[n_views]] uint8 that receives 0 / 1 per pixel.  ONE launch of a fixed grid whatever the scene;
 *                   the workgroup -> (view, tile) mapping is a binary search of pix_start_dev on the device.  The entry point
 *                   allocates nothing, reads nothing back and does no per-view host work; the kernel reads the camera table
 *                   and pix_start and nothing else.
 * Returns NCW_E_BADARG without a launch for NULL cams / pix_start / origin / count, n_views < 1 or radius <= 0 (or NaN).
 * ---------------------------------------------------------------------------------------- */
int ncw_views_roi(const NcwViewCamera* cams_dev, const int64_t* pix_start_dev, int n_views, const float* origin_host, float radius,
                  uint32_t* count_dev, uint8_t* mask_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Checking the alignment (csrc/ncw_gtreproj.hip): the ground-truth reprojection error of SfM tracks, tools/reproj_error.py --
 * the one check of the sfm2gt matrix that the evaluation chain multiplies by.
 *   ncw_pixel_nearest : replaces reproj_error.py:21-51 (get_gt_point), for ALL queries in one pass over the cloud.  For each of
 *                       the n_queries queries of queries_dev (DEVICE table) it finds, among the n points xyz_dev [n,3] f32 (the
 *                       points p0 .. p0 + n - 1 of the cloud), the one nearest to the camera that projects onto the query's
 *                       pixel.  Float32, no contraction, every product and sum rounded in the order written:
 *                           X = rintf(qx);  Y = rintf(qy)                              (torch.round: ties to even)
 *                           c_k = ((w_k0 x + w_k1 y) + w_k2 z) + w_k3                  (k = 0, 1, 2; w = w2c row-major)
 *                           u = (fx c_0 + cx c_2) / c_2;  v = (fy c_1 + cy c_2) / c_2  (IEEE division)
 *                           hit = rintf(u) == X  and  rintf(v) == Y  and  c_2 >= 0
 *                           key = (bits(c_2 + 0.0f) << 32) | (p0 + i)
 *                           best[q] = min(best[q], key)                                (64-bit integer atomicMin)
 *                       c_2 >= 0: the bit pattern orders like the value, so the minimum is the nearest point and equal depths
 *                       resolve to the lowest index.  clear != 0 first fills best_dev [n_queries] uint64 with all-ones on
 *                       `stream`; a query that no point hits keeps all-ones.  The integer minimum does not depend on arrival
 *                       order: the result is bitwise reproducible and bitwise the same for any split of the cloud into launches
 *                       (p0, clear = 0).  No float atomics.  A workgroup owns NCW_PIXNN_WG_POINTS consecutive points in registers
 *                       and walks the queries in LDS tiles of NCW_PIXNN_QUERY_TILE; a division-free bound that is a superset of
 *                       the predicate (argued in the source) keeps the divisions to about one pair in width x height.
 *                       Returns NCW_E_BADARG without a launch for a NULL pointer, n_queries < 1, n < 0, p0 < 0 or
 *                       p0 + n > 2^32 - 1; n == 0 with clear set only clears.
 *   ncw_reproj_errors : replaces reproj_error.py:120-138 (image_reproj_error) and :233-236 (the per-track-element errors):
 *                       err[i] = |(P [p, 1])_xy / (P [p, 1])_z - xy[i]| with P = proj_dev[cam_idx[i]] (3x4 row-major, K [R|t]),
 *                       p = xyz_dev[pt_idx[i]], in float32 without contraction:
 *                           h_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3;  dx = h_0 / h_2 - xy[i][0];  dy = h_1 / h_2 - xy[i][1]
 *                           err[i] = sqrtf(dx dx + dy dy)
 *                       and seg_sum[s] (float64) = the sum of err over the observations seg_start[s] .. seg_start[s + 1] - 1
 *                       (seg_start_dev [n_seg + 1] int64, DEVICE, ascending; clamped to [0, n_obs]).  One wave per segment:
 *                       lane l adds the observations l, l + 64, .. of the segment in sequence in float64, then a fixed xor
 *                       butterfly (32, 16, .. 1) sums the lanes: the order is fixed by the segment alone, so seg_sum is bitwise
 *                       reproducible; an empty segment gives 0.  err is written for the observations inside a segment.  A camera
 *                       or point index outside [0, n_cams) / [0, n_pts) reads nothing and gives NaN.
 *                       Returns NCW_E_BADARG without a launch for a NULL pointer, n_cams < 1, n_pts < 1, n_obs < 0 or n_seg < 0;
 *                       0 without a launch for n_seg == 0.
 * ---------------------------------------------------------------------------------------- */
#define NCW_PIXNN_WG_POINTS 2048
#define NCW_PIXNN_QUERY_TILE 256

typedef struct NcwPixelQuery {
    float w2c[12];          /* world -> camera, 3x4 row-major */
    float fx, fy, cx, cy;
    float qx, qy;           /* the key-point */
} NcwPixelQuery;

int ncw_pixel_nearest(const NcwPixelQuery* queries_dev, int n_queries, const float* xyz_dev, int64_t p0, int64_t n, int clear,
                      uint64_t* best_dev, void* stream);
int ncw_reproj_errors(const float* proj_dev, int n_cams, const float* xyz_dev, int64_t n_pts, const int32_t* cam_idx_dev,
                      const int32_t* pt_idx_dev, const float* xy_dev, int64_t n_obs, const int64_t* seg_start_dev, int64_t n_seg,
                      float* err_dev, double* seg_sum_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Appearance-code fit on frozen geometry (csrc/ncw_appfit.hip; appfit.py).  The reference's dataset hands out every test image
 * as a left half to fit on and a right half to score (datasets/phototourism.py:520-556, 726-748: rays_train / rgbs_train_gt,
 * rays_eval / rgbs_eval_gt) and has no consumer for it; this is that consumer's hot path.  With the weights frozen and
 * perturb = 0 everything but the two colour outputs is a constant of the ray, and the rendered colour is linear in them.
 *   ncw_appfit_loss : one wave per ray, four rays per workgroup.  weights [R, M], inside [R, S], weights_sum [R] are the cached
 *                     outputs of ncw_composite_fwd (M = S + O with bg_rgb, else S); rgb [R*S, 3]; bg_rgb [R*M, 3] or NULL;
 *                     background_rgb: DEVICE float[3] or NULL; target [R, 3].
 *                         color[r]   = sum_j w_j (inside_j ? rgb_j : bg_rgb_j or 0) + background_rgb (1 - weights_sum[r])
 *                                      -- the NcwCompositeOut.color expression of the compositor (renderer.py:751-754) in its
 *                                      lane-strided order and wave reduction: the same bits
 *                         ray_loss[r]= sum_c |color_c - target_c|                       (the caller sums the rays in a fixed order)
 *                         d_rgb      = scale w_j sign(color - target) inv_denom where inside_j, 0 elsewhere        [R*S, 3]
 *                         d_bg_rgb   = the same on the complementary samples (NULL iff bg_rgb is NULL)             [R*M, 3]
 *                     sign(0) = 0 as torch's.  inv_denom = 1 / (R_total + 1e-5): the L1 colour loss of losses.py:25-27 with
 *                     R_total the rays of the WHOLE fit set, not of this launch.  loss_scale: DEVICE float[2] = {scale, 1 / scale}
 *                     (the fp16 mode's pair, NcwCompositeGrad.grad_scale_dev) or NULL = 1.  No atomics.
 *                     Returns NCW_E_BADARG for a NULL pointer, S < 1, O < 0 or bg_rgb / d_bg_rgb not both given; 0 for R == 0.
 *   ncw_appfit_step : sums d_a_rows [n, n_a] (the per-point code adjoints ncw_color_bwd / ncw_nerf_bwd store when given
 *                     d_a_rows) over its n rows into grad_acc [n_a] (accumulate != 0: added to what it holds).  Fixed order:
 *                     workgroup k sums rows [NCW_APPFIT_BLOCK_ROWS k, NCW_APPFIT_BLOCK_ROWS (k + 1)) -- a wave adds its 64 rows
 *                     in sequence, the four waves combine as (w0 + w1) + (w2 + w3) -- into scratch, then ONE workgroup adds the
 *                     block sums to grad_acc in block order.  Bitwise run-to-run reproducible, and bitwise independent of how
 *                     a row sequence is split into accumulating calls as long as every call but the last holds a multiple of
 *                     NCW_APPFIT_BLOCK_ROWS rows (any split of rows whose sums are exact in fp32, e.g. small integers).
 *                     Two back-to-back launches (block sums; one workgroup), nothing is handed between workgroups inside a
 *                     launch; no atomics.  n == 0 is allowed (the final call of an iteration).
 *                     final_call != 0 then, in the same single-workgroup launch: g = grad_acc * loss_scale[1];
 *                       any g non-finite: code and moments untouched, state->skipped += 1, loss_scale halves (>= scale_min);
 *                       otherwise state->step += 1 and one Adam step on code [n_a] (torch.optim.Adam's arithmetic as in
 *                       ncw_adam_step_dev: bias corrections in double, no clipping, no weight decay);
 *                     and on an applied step the new code is broadcast into a_rows [R_rows, n_a] (what ncw_color_fwd /
 *                     ncw_nerf_fwd read per ray).  scratch: ncw_appfit_step_scratch_floats(n, n_a) floats.
 *                     Returns NCW_E_BADARG for n_a outside [1, NCW_APPFIT_MAX_NA], n < 0 or a missing pointer.
 * ---------------------------------------------------------------------------------------- */
#define NCW_APPFIT_BLOCK_ROWS 256
#define NCW_APPFIT_MAX_NA 128
int ncw_appfit_loss(const float* weights, const float* inside, const float* weights_sum, const float* rgb, const float* bg_rgb,
                    const float* background_rgb, const float* target, int R, int S, int O, float inv_denom,
                    const float* loss_scale, float* color, float* ray_loss, float* d_rgb, float* d_bg_rgb, void* stream);
int64_t ncw_appfit_step_scratch_floats(int64_t n, int n_a);
int ncw_appfit_step(const float* d_a_rows, int64_t n, int n_a, float* scratch, float* grad_acc, int accumulate, int final_call,
                    float* code, float* exp_avg, float* exp_avg_sq, NcwAdamState* state, float lr, float beta1, float beta2,
                    float eps, float* loss_scale, float scale_min, float* a_rows, int64_t R_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh operations (csrc/ncw_meshops.hip; meshops.py): connected components of a triangle mesh and the compaction of a face
 * subset.  THE REFERENCE HAS NO SUCH MODE, for any entry point of this section: its reprojection filter writes a point cloud
 * (utils/reproj_filter.py:293-300) and nothing in it labels components; the rules below are this project's.
 * faces [F,3] int32, vertex indices below 2^31; F, V <= 2^31 - 1.
 * CONNECTIVITY IS BY SHARED VERTEX INDEX.  Two faces that only share coordinates are NOT connected; two pieces that touch in
 * one welded vertex ARE one component (trimesh's `split` goes by shared edges, open3d's cluster_connected_triangles by
 * adjacent triangles: no parity with either is claimed).
 * A face PARTICIPATES iff keep[f] != 0 (keep NULL: every face), its three corners lie in [0, V) and are pairwise distinct; the
 * corners of any other face are never used as indices.
 * Integer atomics only (min, add), never float atomics: all results are functions of the mesh, bitwise reproducible and
 * independent of launch order or split.
 *   ncw_mesh_cc_hook     : parent [V] int32 = arange(V) on entry (caller).  One lane per face unions its corners (0, 1) and
 *                          (0, 2) in a lock-free union-find: find the two roots; hook the larger root under the smaller with
 *                          old = atomicMin(&parent[hi], lo); if old != hi, go on with (old, lo).  Invariant parent[x] <= x at
 *                          all times: no cycles, every retry strictly decreases an index.  No lane ever waits on another
 *                          lane's progress: no spin loops, no locks.  Walks halve their path with the same atomicMin.  On return
 *                          (stream order) parent holds one tree per component, root = its smallest vertex index.
 *   ncw_mesh_cc_flatten  : parent[v] = root(v) for every v: labels.  The label of a component is the SMALLEST VERTEX INDEX IN
 *                          IT; a vertex used by no participating face is its own label.
 *   ncw_mesh_cc_sizes    : sizes [V] int32, ZEROED by the caller: sizes[l] = number of participating faces of the component
 *                          with label l (taken at corner 0), 0 at every index that is not such a label.  Integer atomicAdd,
 *                          aggregated per wave (one add per distinct label) and per workgroup (LDS) before global memory.
 *   ncw_mesh_face_select : keep_out [F] uint8 = 1 iff the corners are in range and distinct, AND (vflags != NULL) at least
 *                          min_corners (1..3) corners have vflags [V] uint8 != 0, AND (labels != NULL) comp_ok[labels[corner 0]]
 *                          != 0 (labels [V] int32, comp_ok [V] uint8: both or neither); else 0.  No atomics.
 *   ncw_mesh_compact_mark: used [V] uint8 (ZEROED by the caller): used[v] = 1 for the in-range corners of the faces with
 *                          keep[f] != 0.  Plain stores; all writers store the same value.
 *   (caller)             : vmap = exclusive prefix sum of used, face_offset = exclusive prefix sum of keep (0 / 1 values), both
 *                          int32 (torch.cumsum); n_out = the number of kept faces.
 *   ncw_mesh_compact_faces: faces_out [n_out,3] int32: row face_offset[f] = vmap of the corners of every face with keep[f] != 0
 *                          (a corner outside [0, V) is written as -1 and vmap is not read; a face whose offset lies outside
 *                          [0, n_out) is not written).  Kept vertices and kept faces KEEP THEIR RELATIVE ORDER.
 * All return NCW_E_BADARG without a launch for a missing pointer, F or V outside [0, 2^31 - 1], min_corners outside 1..3, labels
 * and comp_ok not both given, or n_out outside [0, F]; 0 without a launch for an empty range.
 * ---------------------------------------------------------------------------------------- */
int ncw_mesh_cc_hook(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts, int32_t* parent, void* stream);
int ncw_mesh_cc_flatten(int32_t* parent, int64_t n_verts, void* stream);
int ncw_mesh_cc_sizes(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts, const int32_t* labels,
                      int32_t* sizes, void* stream);
int ncw_mesh_face_select(const int32_t* faces, int64_t n_faces, int64_t n_verts, const uint8_t* vflags, int min_corners,
                         const int32_t* labels, const uint8_t* comp_ok, uint8_t* keep_out, void* stream);
int ncw_mesh_compact_mark(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts, uint8_t* used,
                          void* stream);
int ncw_mesh_compact_faces(const int32_t* faces, const uint8_t* keep, const int32_t* face_offset, const int32_t* vmap,
                           int64_t n_faces, int64_t n_verts, int64_t n_out, int32_t* faces_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification (csrc/ncw_simplify.hip; meshops.simplify): uniform-grid vertex clustering with a quadric-optimal
 * representative per cell (Lindstrom, out-of-core simplification).  THE REFERENCE HAS NO SUCH MODE (it leaves decimation to an
 * external tool): the rules below are this project's, and no parity with open3d's simplify_vertex_clustering, trimesh or
 * meshlab is claimed.  Restated in numpy by tests/_simplify_ref.py.
 * verts [V,3] float64 (float32 input is converted exactly by the caller), faces [F,3] int32, cell size h > 0 (float64),
 * eps (default 1e-3).  ALL ARITHMETIC IS FLOAT64, EVERY PRODUCT, SUM AND QUOTIENT ROUNDED ON ITS OWN (no fused multiply-add),
 * every sum sequential in the stated order, one lane per sum.  No float atomics: bitwise reproducible.
 *  1 PARTICIPATION  A face takes part iff its corners lie in [0, V) and are pairwise distinct (ncw_mesh_face_select's rule).
 *                   A vertex is USED iff a participating face names it (ncw_mesh_compact_mark of those faces).
 *  2 GRID           lo, hi = componentwise min / max over the used vertices (caller, exact).  n = floor((hi - lo) / h) + 1 per
 *                   axis.  Cell index i = clamp(floor((x - lo) / h), 0, n - 1) per axis -- a division, so a coordinate with
 *                   x - lo = k h exactly goes to the upper cell k.  key = (i_x n_y + i_y) n_z + i_z, int64.  The caller refuses
 *                   n_x n_y n_z >= 2^62, h not finite and positive, non-finite lo / hi, and a mesh with no participating face.
 *                   Cell centre c = lo + (i + 0.5) h  (i + 0.5 exact, then the product, then the sum).
 *  3 CLUSTERS       The distinct keys of used vertices in ascending order, numbered 0 .. C-1 (caller).  cluster [V] int32 holds
 *                   the number of a used vertex and -1 for an unused one.
 *  4 MEMBER MEAN    m_k = (sum of (x_v - c_k) over the used vertices of cluster k in ascending v, from 0.0) / count.
 *  5 QUADRIC        A participating face contributes to cluster k ONCE per distinct cluster among its corners: corner j
 *                   contributes iff its cluster differs from the clusters of the corners before it.  With P_i = x_i - c_k for
 *                   the face's corners i = 0, 1, 2 in the face's own order:
 *                       u = P_1 - P_0, w = P_2 - P_0, n = u x w = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x),
 *                       d = (n_x P_0x + n_y P_0y) + n_z P_0z,
 *                       A_00 += n_x n_x, A_01 += n_x n_y, A_02 += n_x n_z, A_11 += n_y n_y, A_12 += n_y n_z, A_22 += n_z n_z,
 *                       b += d n,
 *                   from 0.0, over the cluster's faces in ascending face index.  A zero-area face adds zeros.
 *  6 PLACEMENT      t = (A_00 + A_11) + A_22.  t == 0: p = m.  Otherwise lam = (eps t) / 3, M = A + lam I, r = b + lam m and
 *                   p = M^-1 r by cofactors, in this order:
 *                       c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
 *                       c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01,
 *                       det = (M00 c00 + M01 c01) + M02 c02,
 *                       p_0 = ((c00 r_0 + c01 r_1) + c02 r_2) / det,  p_1 = ((c01 r_0 + c11 r_1) + c12 r_2) / det,
 *                       p_2 = ((c02 r_0 + c12 r_1) + c22 r_2) / det.
 *                   If det is not finite or not > 0, or some |p_i| <= h / 2 does not hold (p outside the cell, or NaN): p = m.
 *                   Output vertex c_k + p; at_mean[k] = 1 iff p = m was taken (t == 0 included).
 *  7 FACES          A participating face SURVIVES iff its three clusters are distinct.  It is rotated, not reflected, so that
 *                   its smallest cluster comes first.  Survivors with equal rotated triples are duplicates and the one with the
 *                   smallest input index is kept (caller: stable sorts); a pair of OPPOSITE orientation is not a duplicate,
 *                   both stay.  Output faces in ascending input index.
 *  8 OUTPUT         Only the clusters some kept face names, ascending (caller: meshops.submesh).  All faces collapsing gives
 *                   the empty mesh.
 *  9 COLOURS        (optional, uint8 [V,3]) per cluster and channel floor(sum / count + 0.5) over its used members; integer
 *                   sums, computed as (2 sum + count) / (2 count) in integers.
 * Clustering can create non-manifold edges and joins components that come within one cell of each other.
 *   ncw_mesh_sc_keys  : keys [V] int64 = the key of every vertex with used[v] != 0, -1 elsewhere.  lo [3] and n [3] are HOST
 *                       pointers.
 *   ncw_mesh_sc_faces : per face: tri [F,3] int32 = the rotated cluster triple of a survivor, (-1, -1, -1) otherwise;
 *                       survive [F] uint8; inc [F,3] int32 = per corner the cluster the face contributes to (rule 5), -1
 *                       where it does not (every corner of a face that takes no part).
 *   (caller)          : CSR per cluster by stable sorts: mem [n_mem] int32 = the used vertices by cluster, ascending v within
 *                       one; inc [n_inc] int32 = the FACE index of the inc entries >= 0 by cluster, ascending face within one;
 *                       mem_off / inc_off [C+1] int64; keys [C] int64 = the cluster's key.
 *   ncw_mesh_sc_place : one lane per cluster, rules 4, 5, 6, 9: out_verts [C,3] float64, at_mean [C] uint8, out_colors [C,3]
 *                       uint8 (colors and out_colors both or neither).  List entries outside [0, V) / [0, F), faces that take
 *                       no part and offsets outside the lists are skipped, never used as indices.
 * All return NCW_E_BADARG without a launch for a missing pointer, counts outside their ranges (V, F <= 2^31 - 1, C <= V,
 * n_mem <= V, n_inc <= 3 F), a grid the caller must refuse (above; n < 1), eps negative or not finite; 0 without a launch for an
 * empty range.
 * ---------------------------------------------------------------------------------------- */
int ncw_mesh_sc_keys(const double* verts, const uint8_t* used, int64_t n_verts, const double* lo, double h, const int64_t* n,
                     int64_t* keys, void* stream);
int ncw_mesh_sc_faces(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* cluster, int64_t n_clusters,
                      int32_t* tri, uint8_t* survive, int32_t* inc, void* stream);
int ncw_mesh_sc_place(const double* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int64_t* keys,
                      int64_t n_clusters, const int64_t* mem_off, const int32_t* mem, int64_t n_mem, const int64_t* inc_off,
                      const int32_t* inc, int64_t n_inc, const double* lo, double h, const int64_t* n, double eps,
                      const uint8_t* colors, double* out_verts, uint8_t* at_mean, uint8_t* out_colors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Estimating sfm2gt (csrc/ncw_align.hip; align.icp_similarity): the two kernels of a gated point-to-point ICP with a similarity
 * transform (Umeyama), source = the filtered SfM points P [N,3] float64, target = the ground-truth cloud Q [M,3] float64,
 * bucketed ONCE by the caller (evalmesh.NNGrid over float32(Q - centre)); the source is transformed every iteration, the target
 * never.  THE REFERENCE HAS NO SUCH TOOL (heritage-recon ships the matrices): the rules below are this project's, and no parity
 * with open3d / CloudCompare registration is claimed.  Restated in numpy by tests/_align_ref.py.
 * ALL ARITHMETIC IS FLOAT64 UNLESS SAID OTHERWISE, EVERY PRODUCT AND SUM ROUNDED ON ITS OWN (no fused multiply-add).  No float
 * atomics: bitwise reproducible.  T [12]: a 3x4 row-major matrix (rows of sR | t), a HOST pointer, as are centre, box_lo,
 * box_hi, cp and cq.
 *  1 TRANSFORM      x_a = ((T[4a] p_x + T[4a+1] p_y) + T[4a+2] p_z) + T[4a+3]   for a = 0, 1, 2.
 *  2 QUERY          q32_a = (float)(x_a - centre_a): one float64 subtraction, one rounding to float32.
 *  3 INSIDE         inside = 1 iff for every axis  q32_a >= box_lo_a - gate  and  q32_a <= box_hi_a + gate, the two bounds and the
 *                   comparisons in float32 (box_lo / box_hi: the target's box, recentred, float32); 0 if a coordinate is NaN.
 *                   A point that is not inside has no partner within the gate: the caller does not query it and gives it
 *                   idx = -1.  |q32| of every queried point is at most the box's half-extent plus the gate.
 *  4 PAIRS          Pair i takes part iff 0 <= idx[i] < M and dist[i] <= gate (float32, inclusive; a NaN dist takes no part).
 *  5 TERMS          With p = P[i] - cp, q = Q[idx[i]] - cq (componentwise), x = rule 1 of P[i], d = x - Q[idx[i]]:
 *                       s[0..2] += p_a,   s[3..5] += q_a,   s[6 + 3a + b] += p_a q_b,
 *                       s[15] += (p_x p_x + p_y p_y) + p_z p_z,   s[16] += (q_x q_x + q_y q_y) + q_z q_z,
 *                       s[17] += (d_x d_x + d_y d_y) + d_z d_z  (= r2),
 *                       s[18] += (double)dist[i],   s[19] += (double)dist[i] (double)dist[i],
 *                   counts[0] += 1 (int64), counts[1] = max(counts[1], bit pattern of r2 as int64) over the pairs whose r2 is
 *                   not NaN (a non-negative double orders like its bit pattern), from 0.
 *  6 ORDER          L = NCW_ALIGN_LANES lanes, B = NCW_ALIGN_BLOCK points per block, ceil(N / B) blocks.  Block b, lane l adds
 *                   the terms of the points b B + j L + l for j = 0, 1, .. B / L - 1 (those below N that take part) in ascending
 *                   j, each of the 20 sums on its own from 0.0.  LANE TREE: v[l] = v[l] + v[l + s] for s = 32, 16, 8, 4, 2, 1
 *                   inside every group of 64 consecutive lanes (l mod 64 < s), leaving the group sums w_0 .. w_3 on lanes 0, 64,
 *                   128, 192; the block's row is (w_0 + w_1) + (w_2 + w_3).  FOLD: one workgroup of L lanes, lane l adds the
 *                   rows l, l + L, l + 2 L, .. in ascending order from 0.0, then the same lane tree.  The result is a function
 *                   of N and the data only.
 *   ncw_align_transform  : rules 1-3 for n points: q32 [n,3] float32, inside [n] uint8.
 *   ncw_align_sums_blocks: ceil(n / NCW_ALIGN_BLOCK), 0 for n <= 0: the rows of scratch the caller provides.
 *   ncw_align_sums       : rules 4-6: sums [20] float64, counts [2] int64; scratch part [blocks, 20] float64, ipart [blocks, 2]
 *                          int64 (both may be NULL when n == 0, as may src / idx / dist).  n == 0 gives zeros.
 * Both return NCW_E_BADARG without a launch for a missing pointer, n outside [0, 2^31 - 1] or m < 0; ncw_align_transform
 * returns 0 without a launch for n == 0.
 * ---------------------------------------------------------------------------------------- */
#define NCW_ALIGN_LANES 256
#define NCW_ALIGN_BLOCK 1024
#define NCW_ALIGN_SUMS 20
int ncw_align_transform(const double* src, int64_t n, const double* T, const double* centre, const float* box_lo,
                        const float* box_hi, float gate, float* q32, uint8_t* inside, void* stream);
int64_t ncw_align_sums_blocks(int64_t n);
int ncw_align_sums(const double* src, int64_t n, const double* cp, const double* dst, int64_t m, const double* cq,
                   const int64_t* idx, const float* dist, float gate, const double* T, double* part, int64_t* ipart,
                   double* sums, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fusing traced surface samples into one surface cloud (csrc/ncw_fuse.hip; surfcloud.SurfaceCloud / fuse_views): the hits of
 * many sphere-traced views (ncw_trace_*), each with the SDF gradient and the colour network's answer, are accumulated per cell
 * of a uniform grid in an open-addressed device table and resolved to one oriented, coloured point per occupied cell.  THE
 * REFERENCE HAS NO SUCH TOOL: cell rule, filters and rounding below are this project's, and no parity with open3d's
 * voxel_down_sample or any multi-view-stereo fusion is claimed.  Restated in numpy by tests/_fuse_ref.py.
 * A sample i of the view with serial v (0 <= v <= NCW_FUSE_MAX_SERIAL): point p [3] f32 in the network's unit-sphere frame,
 * gradient n [3] f32 (unnormalised), ray direction d [3] f32 (|d| = 1 as the ray kernels write it), colour c [3] f32.
 * Grid (NcwFuseGrid, a HOST struct): lo [3], cell size h > 0, dims [3] each in 1 .. 2^20, the frame change x = p scale + off,
 * cos_min and the facing switch.  ALL ARITHMETIC BELOW IS FLOAT64 (f32 inputs converted exactly), EVERY PRODUCT, SUM AND
 * QUOTIENT ROUNDED ON ITS OWN (no fused multiply-add), divisions and square roots IEEE.
 *  1 QUANTISE    x_a = (double)p_a scale + off_a;  g_a = (x_a - lo_a) / h;  cell_a = floor(g_a).  The sample is VALID iff
 *                  - every p_a, n_a, d_a is finite,
 *                  - 0 <= cell_a < dims_a on all axes,
 *                  - nn = (n_x n_x + n_y n_y) + n_z n_z is finite and > 0,
 *                  - facing != 0:  -((n_x d_x + n_y d_y) + n_z d_z) >= cos_min sqrt(nn)   (facing == 0: no such test).
 *                key = (cell_z dims_y + cell_y) dims_x + cell_x (int64); an invalid sample has key -1 and adds nothing.
 *                Payload, all integers:  qpos_a = min((int)floor((g_a - cell_a) 65536), 65535);
 *                qn_a = llrint(n_a / sqrt(nn) * 32767) (the quotient, then the product; ties to even);
 *                qc_a = llrint(min(max(c_a, 0), 1) * 255), a NaN colour giving 0.
 *  2 ACCUMULATE  Per key the table holds acc [NCW_FUSE_ACC] int64 = count, sum qpos [3], sum qn [3], sum qc [3], and views
 *                int32 = the number of DISTINCT serials that contributed.  Only integers are added: the content is a function
 *                of the multiset of (sample, serial) pairs alone -- not of sample order, of how a view's samples are split
 *                into calls, or of the run.  (WHERE in the table a key sits does depend on the run; nothing reads that.)
 *  3 RESOLVE     One lane per occupied cell, cells in ascending key (the caller's row list).  With S = sum qpos, N = sum qn:
 *                  pos_a = lo_a + ((double)cell_a + ((double)S_a / (double)count + 0.5) / 65536.0) h,
 *                  L = sqrt((N_x N_x + N_y N_y) + N_z N_z);  L == 0: normal = 0 and degenerate = 1, else
 *                  normal_a = (float)(N_a / L);
 *                  colour_a = (2 sum qc_a + count) / (2 count) in integers (rule 9 of the mesh simplification).
 *                Every position lies strictly inside its cell (the mean offset is in [0.5, 65535.5] / 65536).
 * THE TABLE (NcwFuseTable, a HOST struct of device pointers): capacity = a power of two; keys [capacity] int64, NCW_FUSE_EMPTY
 * in a free slot; acc [capacity, NCW_FUSE_ACC] int64; stamp, views [capacity] int32; counters [NCW_FUSE_COUNTERS] int64
 * (occupied slots, dropped samples, valid samples).  The caller creates it with keys = EMPTY and everything else 0.
 * Open addressing, linear probing from a 64-bit mix of the key (splitmix64's finaliser) masked to the capacity; an EMPTY word
 * is claimed by compare-and-swap; the payload goes in by integer atomic adds; old = atomicMax(&stamp, v + 1) and views += 1 iff
 * old < v + 1 -- correct because the caller hands out serials that NEVER DECREASE (samples of one serial may arrive in several
 * calls).  The probe loop is bounded by the capacity: a sample that finds neither its key nor an EMPTY word adds 1 to
 * counters[NCW_FUSE_CNT_OVERFLOW] and is dropped (the caller keeps the table at most half full and turns a non-zero counter
 * into an error).  No lane waits for another (no spin, no lock, no flag hand-off).  While a launch inserts, every word of the
 * table is touched only by agent-scope atomics or relaxed agent-scope atomic loads -- no plain loads or stores (the L2s of the
 * XCDs are not coherent for those) -- and there are no float atomics.  The counters are summed per wave before one atomic.
 *   ncw_fuse_insert  : rules 1, 2 for n samples of serial `serial` in ONE launch, one lane per sample.
 *   ncw_fuse_move    : every occupied row of src is added into dst (capacity >= src's, different storage) by the same
 *                      find-or-claim and atomics; dst's stamp = max, views += src's views (a key is in src once).  dst's
 *                      occupied / overflow counters count what the move did; the valid counter is the caller's to carry.
 *   (caller)         : rows [C] int64 = the slots with keys >= 0, sorted by their key ascending (torch.nonzero / torch.sort).
 *   ncw_fuse_resolve : rule 3 for the C rows: pos [C,3] f64, normal [C,3] f32, colour [C,3] u8, count [C] int64, views [C]
 *                      int32, degenerate [C] u8, keys [C] int64.  A row outside [0, capacity) or without a key of this grid
 *                      gives zeros, degenerate 1 and key -1, and is never used as an index.
 * All return NCW_E_BADARG without a launch for a missing or misaligned pointer (8 bytes for 64-bit words, 4 for 32-bit), n
 * outside [0, 2^31 - 1], a serial outside [0, NCW_FUSE_MAX_SERIAL], a capacity that is not a power of two in
 * [1, 2^NCW_FUSE_MAX_CAPACITY_LOG2], n_rows > capacity, h not finite and > 0, lo / scale / off (and cos_min when facing) not
 * finite, or a dimension outside [1, 2^NCW_FUSE_MAX_DIM_LOG2]; 0 without a launch for an empty range.
 * ---------------------------------------------------------------------------------------- */
#define NCW_FUSE_ACC 10
#define NCW_FUSE_COUNTERS 4
#define NCW_FUSE_CNT_OCCUPIED 0
#define NCW_FUSE_CNT_OVERFLOW 1
#define NCW_FUSE_CNT_VALID 2
#define NCW_FUSE_EMPTY (-1)
#define NCW_FUSE_MAX_DIM_LOG2 20
#define NCW_FUSE_MAX_CAPACITY_LOG2 36
#define NCW_FUSE_MAX_SERIAL 0x7ffffffe
typedef struct NcwFuseGrid {
    double lo[3];
    double h;
    int64_t dims[3];
    double scale;
    double off[3];
    double cos_min;
    int32_t facing; /* 0: the facing test is switched off */
    int32_t _pad;
} NcwFuseGrid;
typedef struct NcwFuseTable {
    int64_t* keys;
    int64_t* acc;
    int32_t* stamp;
    int32_t* views;
    int64_t* counters;
    int64_t capacity;
} NcwFuseTable;
int ncw_fuse_insert(const float* points, const float* grads, const float* dirs, const float* colours, int64_t n, int32_t serial,
                    const NcwFuseGrid* grid, const NcwFuseTable* table, void* stream);
int ncw_fuse_move(const NcwFuseTable* src, const NcwFuseTable* dst, void* stream);
int ncw_fuse_resolve(const NcwFuseTable* table, const int64_t* rows, int64_t n_rows, const NcwFuseGrid* grid, double* pos,
                     float* normal, uint8_t* colour, int64_t* count, int32_t* views, uint8_t* degenerate, int64_t* keys,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic scenes with known ground truth (csrc/ncw_synth.hip; neuralrecon-w_amd/synth.py).  Replaces nothing in the reference:
 * it has no scene generator, its scenes are downloaded.  These two launches make, from a triangle mesh, what a photo collection
 * and its SfM model give the pipeline: the image with its semantic map, and the key-point observations of one view.  Both run one
 * lane per output element, without atomics, LDS or transcendental functions; every product, sum and quotient is rounded once
 * (IEEE, no fused multiply-add), so tests/_synth_ref.py restates them in numpy bit for bit.  What needs a square root is handed in
 * by the host (unit face normals, sigma sqrt(3)).
 *
 *   ncw_synth_shade   : deferred shading of ONE image from the depth / face planes ncw_raster_resolve wrote at ss x ss samples
 *                       per pixel (depth_ss, face_ss: [height ss][width ss], ss in 1..NCW_SYNTH_MAX_SS).
 *       Pixel convention: the project's rays go through INTEGER pixel coordinates (ncw_view_rays: dir = ((c - cx) / fx, ..)),
 *       the rasterizer samples at (c + 0.5, r + 0.5).  The image written here is the one those rays see: sub-sample (i, j) of
 *       pixel (r, c) sits at image point (c + (i + 0.5) / ss - 0.5, r + (j + 0.5) / ss - 0.5), and the caller rasterizes the
 *       (height ss) x (width ss) planes with fx ss, fy ss, cx ss + 0.5 ss, cy ss + 0.5 ss.  img->fx .. cy are those of the
 *       height x width image itself.
 *       Per sub-sample with a face f in [0, n_faces): camera point (x d, y d, d) with x = (px - cx) / fx, y = (py - cy) / fy
 *       (OpenCV axes) -> world through c2w -> GT frame through sfm2gt (both row-major 3x4, float32, a b + c d + e f + g left to
 *       right).  albedo[c] = base[c] (1 + amp (n - 0.4375)), n = n0 / 2 + n1 / 4 + n2 / 8, n_o = value noise of the GT point
 *       times freq 2^o: the lattice value at integer (ix, iy, iz) is (w >> 8) 2^-24 with w = word 0 of Philox4x32-10 of counter
 *       (ix, iy, iz, tex_seed) and key (o, 0), interpolated trilinearly (x, then y, then z) as a + t (b - a); lattice
 *       coordinates are clamped to +-2^30.  Flat Lambert: s = ambient + diffuse max(0, normal[f] . light) (normal: unit, the
 *       caller's frame; light: unit, the same frame).  v[c] = clamp(gain[c] albedo[c] s + bias[c], 0, 1).  A sub-sample without a
 *       face (face < 0 or >= n_faces, or depth <= 0) takes sky_top + t (sky_bottom - sky_top), t = r / height, clamped likewise.
 *       rgb[r][c][ch] = uint8(mean 255 + 0.5) by truncation, the mean taken in (j, i) order and divided by ss ss; label[r][c] and
 *       depth[r][c] are those of sub-sample (ss / 2, ss / 2): the material's label (sky_label without a face), the depth (0).
 *       materials[n_materials] on the device, indexed by face_material[f] (uint8, clamped to n_materials - 1); 1 <= n_materials
 *       <= 256.  height width ss ss < 2^31.
 *   ncw_synth_observe : key-point observations of ONE view of n points (pts, nrm: float64 [n][3], world frame, nrm unit; index:
 *       int64 [n], the point's identity).  (x, y, z) = w2c p (row-major 3x4 float64); in front when z > znear; u = fx (x / z) + cx,
 *       v = fy (y / z) + cy; facing when nrm . (centre - p) > 0; the observed pixel (floor(u + 0.5), floor(v + 0.5)) of the
 *       NOISE-FREE projection must lie in the image; visible when depth[row][col] > 0 and |z - depth| <= depth_tol z (depth: the
 *       float32 [height][width] plane ncw_synth_shade wrote, occluders included).  Noise per axis: sigma_r3 (u1 + u2 + u3 + u4 - 2),
 *       sigma_r3 = sigma sqrt(3) from the host: mean 0, variance sigma^2, |noise| <= 2 sqrt(3) sigma.  u_k = (w >> 8) 2^-24 of
 *       the words of Philox4x32-10 with key (seed, seed >> 32) and counters (index, index >> 32, serial, 0) for x and
 *       (.., 1) for y: a draw depends on the point's index and the view's serial alone, never on n or the launch.
 *       xy[n][2] = (u, v) + noise, err2[n] = the SQUARED pixel distance of the noisy from the true projection (the caller takes
 *       the root), vis[n] = 1 / 0.  A point with z <= znear writes xy = 0, err2 = 0, vis = 0.
 * Return codes: 0; NCW_E_BADARG for a NULL pointer, ss outside 1..NCW_SYNTH_MAX_SS, an empty or too large image, n_materials
 * outside 1..256, non-positive fx / fy / znear, negative sigma_r3 / depth_tol; n <= 0 (observe) returns 0 at once.
 * ---------------------------------------------------------------------------------------- */
#define NCW_SYNTH_MAX_SS 4
typedef struct NcwSynthMaterial {
    float base[3];  /* base colour, linear [0, 1] */
    float freq;     /* lattice cells per GT unit of the first octave */
    float amp;      /* texture amplitude */
    int32_t label;  /* ADE20K label id written to the label plane (0..255) */
} NcwSynthMaterial;
typedef struct NcwSynthImage {
    float fx, fy, cx, cy;
    float c2w[12];
    float sfm2gt[12];
    float light[3];
    float ambient, diffuse;
    float gain[3], bias[3];
    float sky_top[3], sky_bottom[3];
    int32_t height, width, ss;
    int32_t sky_label;
    uint32_t tex_seed;
    int32_t _pad;
} NcwSynthImage;
typedef struct NcwSynthView {
    double w2c[12];
    double centre[3];
    double fx, fy, cx, cy;
    double znear;
    double sigma_r3;
    double depth_tol;
    uint64_t seed;
    int32_t height, width;
    uint32_t serial;
    int32_t _pad;
} NcwSynthView;
int ncw_synth_shade(const float* depth_ss, const int32_t* face_ss, const NcwSynthImage* img, const float* face_normal,
                    const uint8_t* face_material, int64_t n_faces, const NcwSynthMaterial* materials, int32_t n_materials,
                    uint8_t* rgb, uint8_t* label, float* depth, void* stream);
int ncw_synth_observe(const double* pts, const double* nrm, const int64_t* index, int64_t n, const NcwSynthView* view,
                      const float* depth, double* xy, double* err2, uint8_t* vis, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth and normal maps against ground truth (csrc/ncw_depthmetrics.hip; depthmetrics.compare_planes): the 2-D scores of ONE
 * view -- abs-rel, RMSE, delta < 1.25^k, angular error and its shares, per-view completeness -- from two device planes, in one
 * launch plus one fold.  THE REFERENCE HAS NO SUCH EVALUATION: the rules below are this project's, and no parity with any
 * published depth benchmark's script is claimed.  Restated in numpy by tests/_depthmetrics_ref.py.
 * ALL PER-PIXEL ARITHMETIC IS FLOAT32, EVERY OPERATION ROUNDED ONCE (no fused multiply-add, IEEE division and square root).  No
 * float atomics: bitwise reproducible.  The kernel calls no transcendental function: thresholds and edge tables come from the
 * host.  Pixel i = row * width + col; n = height * width.
 *  1 INPUTS         gt_z [n] f32 (eye-space z, 0 = empty), gt_n [3][n] f32 unit normals or NULL, pred [n] f32, pred_n [3][n] f32 or
 *                   NULL, mask [n] uint8 or NULL (non-zero = the pixel takes no part).
 *                   mode NCW_DM_PRED_Z: pred is an eye-space z plane (z_p = pred), pred_n holds normals.
 *                   mode NCW_DM_PRED_T: pred is views.trace_view's `depth` (t along the unit ray, unit-sphere units) and pred_n its
 *                   encoded `normal` plane, decoded as 2 v - 1;  z_p = (t * scale) / nrm  with nrm = |d| of ncw_view_rays'
 *                   un-normalised direction of the pixel (ncw_raymath.h, evaluated under rule "rounded once"; its camera-space
 *                   z is -1, so z_p is the eye-space depth of the hit) and scale = the renderer's radius.
 *  2 VALID          gt: gt_z finite and > 0.  prediction: pred finite and > 0 (PRED_T: and z_p finite and > 0).
 *  3 CLASSES        A masked pixel counts as `masked` and nothing else.  Every other pixel is exactly one of both / gt_only
 *                   (the surface is missing here) / pred_only (surface where the truth has none) / neither.
 *  4 TERMS (both)   e = z_p - z_g,  a = |e|,  r = a / z_g,  q = max(z_p / z_g, z_g / z_p),  ee = e e,  s = ee / z_g.
 *                   float64 sums 0..4 += a, e, ee, r, s (each formed in float32, then widened).  delta_k += (q < delta_thr[k]).
 *                   hist_rel[b] += 1 with b = the number of rel_edges <= r (rel_edges [NR] f32, strictly ascending; b in 0..NR).
 *  5 NORMALS        Scored on `both` pixels when gt_n and pred_n are given and both (decoded) normals are finite in every
 *                   component and not (0, 0, 0):  dot = (x x' + y y') + z z',  c = dot < -1 ? -1 : (dot > 1 ? 1 : dot)  (a NaN dot,
 *                   which takes overflowing products, stays NaN).  float64 sum 5 += c, normal count += 1, ang_k += (c >=
 *                   cos_thr[k]), hist_cos[b] += 1 with b = the number of cos_edges > c (cos_edges [NA] f32, strictly descending;
 *                   with edges cos(k D), k = 1..NA, that is floor(angle / D) off the edges: bin k holds the angles in (k D, (k + 1) D],
 *                   bin 0 also the angle 0).
 *  6 PLANES         optional outputs [n] f32: err_rel = r (NaN where not both), err_cos = c (NaN where not scored), z_pred = z_p
 *                   where the prediction is valid, else 0 (masked pixels included).
 *  7 ORDER          L = NCW_DM_LANES lanes, B = NCW_DM_BLOCK pixels per block, ceil(n / B) blocks.  Block b, lane l adds the terms
 *                   of the pixels b B + j L + l, j = 0 .. B / L - 1, in ascending j, each sum on its own from 0.0; then the LANE
 *                   TREE and the FOLD of ncw_align_sums (rule 6 there), word for word.  Counts and histograms are integers.
 *  8 ROW            row v of table [V][K] (8-byte words), K = NCW_DM_FIXED + (NR + 1) + (NA + 1):  words 0..5 the float64 sums
 *                   (a, e, ee, r, s, c) as bit patterns;  6..10 int64 both, gt_only, pred_only, neither, masked;  11..13 delta_1..3;
 *                   14 normal count;  15..17 ang_1..3;  then hist_rel [NR + 1], then hist_cos [NA + 1] (int64).  The entry point
 *                   zeroes the histogram words of row v on the stream; no other row is touched.
 *   ncw_depthmetrics_scratch_bytes : bytes of scratch for a view of n_pix pixels (8-byte aligned; contents need no initialisation).
 *   ncw_depthmetrics_view          : rules 1-8.  prm: HOST struct; its two tables are DEVICE pointers.
 * Returns NCW_E_BADARG without a launch for a NULL gt_z / pred / prm / scratch / table / edge table, height or width < 1, row
 * < 0, another mode, NA or NR outside 1..NCW_DM_MAX_EDGES, row_words != K, scale not finite and > 0, misaligned scratch / table,
 * or (PRED_T) a camera whose size is not the planes'.
 * ---------------------------------------------------------------------------------------- */
#define NCW_DM_PRED_Z 0
#define NCW_DM_PRED_T 1
#define NCW_DM_LANES 256
#define NCW_DM_BLOCK 2048
#define NCW_DM_SUMS 6
#define NCW_DM_COUNTS 12
#define NCW_DM_FIXED 18
#define NCW_DM_MAX_EDGES 2048
typedef struct NcwDepthMetricsParams {
    NcwViewCamera cam;      /* NCW_DM_PRED_T only: fx, fy, cx, cy, c2w, width, height (near / far unused) */
    float scale;
    float delta_thr[3];     /* 1.25, 1.25^2, 1.25^3 rounded to float32 by the caller */
    float cos_thr[3];       /* cos of 11.25, 22.5, 30 degrees likewise */
    int32_t n_cos_edges;    /* NA */
    int32_t n_rel_edges;    /* NR */
    int32_t _pad;
    const float* cos_edges; /* device, [NA] */
    const float* rel_edges; /* device, [NR] */
} NcwDepthMetricsParams;
int64_t ncw_depthmetrics_scratch_bytes(int64_t n_pix);
int ncw_depthmetrics_view(const float* gt_z, const float* gt_n, const float* pred, const float* pred_n, const uint8_t* mask,
                          int height, int width, int mode, const NcwDepthMetricsParams* prm, void* scratch, int64_t* table,
                          int64_t row, int64_t row_words, float* err_rel, float* err_cos, float* z_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif
