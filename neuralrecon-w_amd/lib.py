"""ctypes binding of libneuconw_hip.so (C ABI declared in include/neuconw_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent this
module raises -- a GPU box must run the hand-written HIP kernels or nothing.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# NEUCONW_HIP_LIB: another build of the SAME library (experiment variants from build.py NCW_BUILD_TAG)
LIB_PATH = os.environ.get("NEUCONW_HIP_LIB") or os.path.join(HERE, "libneuconw_hip.so")

PREC_F32 = 0
PREC_BF16 = 1
PREC_F16 = 2  # fp16 operands, f32 accumulate; backward needs the loss scale (renderer.grad_scale)
MAX_LAYERS = 12
MAX_SEGS = 4
ABI_VERSION = 41  # 41: IMLS values of an oriented cloud on a sparse lattice (ncw_imls_values);  40: per-view depth / normal scores against ground truth (ncw_depthmetrics_view / _scratch_bytes, NcwDepthMetricsParams);  39: synthetic scenes (ncw_synth_shade / ncw_synth_observe, NcwSynthMaterial, NcwSynthImage, NcwSynthView);  38: k nearest neighbours and per-point PCA (ncw_knn_query / ncw_knn_pca);  37: surface-cloud fusion (ncw_fuse_insert / _move / _resolve, NcwFuseGrid, NcwFuseTable);  36: sphere tracing (ncw_trace_begin / _step / _finish / _store / _scratch_bytes);  35: nearest point within a radius (ncw_nn_coarse / ncw_nn_query_within);  34: marching cubes on brick-blocked sparse values (ncw_mcs_neighbors / _count / _cube_ids / _emit);  33: sfm2gt estimation (ncw_align_transform / ncw_align_sums / ncw_align_sums_blocks);  32: mesh simplification (ncw_mesh_sc_keys / _sc_faces / _sc_place);  31: ray source (ncw_source_batch, NcwSourceRec, NcwSourceImage);  30: mesh operations (ncw_mesh_cc_hook / _cc_flatten / _cc_sizes / _face_select / _compact_mark / _compact_faces);  29: appearance-code fit on frozen geometry (ncw_appfit_loss / ncw_appfit_step / ncw_appfit_step_scratch_floats);  28: floor-normal loss (NcwCompositeGrad.d_normals, ncw_ray_floor_fwd / _bwd);  27: exact point-to-triangle-mesh distances of the mesh evaluation (ncw_ptm_pack / _count / _emit / _ranges / _cell_keys / _query / _brute, NcwPtmGrid);  26: ground-truth reprojection error of SfM tracks (ncw_pixel_nearest / ncw_reproj_errors, NcwPixelQuery);  25: view selection of the split writer (ncw_views_roi);  24: voxel first-hit views of the reprojection filter's point-cloud source (ncw_voxel_view_seen / ncw_voxel_points_seen, NcwVoxelView);  23: area-weighted surface sampling of the mesh evaluation (ncw_surf_weights / ncw_surf_pick / ncw_surf_sample);  22: ray cache rows (ncw_sfm_depth_splat / ncw_cache_rows, NcwCacheOctree);  21: camera views (ncw_view_rays / ncw_view_store / ncw_image_minmax / ncw_depth_colormap / ncw_image_sqerr / ncw_image_ssim, NcwViewCamera);  20: triangle depth rasterizer of the reprojection filter (ncw_raster_small / _large / _resolve / _backproject / _mark, NcwRasterView);  19: exact 1-NN of the mesh evaluation (ncw_nn_cell_keys / ncw_nn_cell_ranges / ncw_nn_query / ncw_nn_brute, NcwNnGrid);  18: NcwSdfStash.s = residuals of h (adj_mode 2), NcwSdfNet.adj_mode, NcwColorNet.act_split;  17: ncw_ray_voxel_trace (all ray / voxel intersections: kaolin's unbatched_raytrace contract);  16: NcwSdfNet.wt_lo (adjoint sweep with hi + lo weights), NcwNerfNet.w_*_lo;  15: forward-only render form of ncw_sdf_fwd / ncw_color_fwd / ncw_nerf_fwd (NULL stash members);  14: NcwColorNet.w_*_lo (split colour weights, forward);  13: NcwNerfStash.aux_bias;  12: ncw_aux_ray_bias, NcwColorStash.aux_bias, ncw_source_hash;  11: marching cubes (ncw_mc_count / ncw_mc_emit replace the marching-tetrahedra entry points);  10: split-precision SDF value path (NcwSdfNet.w_lo, NcwPackDesc.residual);  9: device-resident optimiser state (ncw_adam_step_dev, NcwAdamState), dynamic loss scale (grad_scale_dev / grad_mul_dev);  8: NcwPoints mode 4 (idx / count), NcwWgradDesc.n_points_dev, ncw_bg_select;  7: fp16 (prec 2), grad_scale / grad_mul;  6: ray prologue / inv_s / loss launches, NcwCompositeOut.weights_max;  5: ncw_scatter_add_rows;  4: ncw_batch_assemble;  3: ordered fp32 wgrad, d_a_rows / ncw_ray_sum_rows, per-ray d_inv_s;  2: 2: NcwWgradDesc.ksplit/n_points, NcwCompositeIn.cos_anneal_dev, ray tail / mesh / optimiser entry points


class NcwSeg(C.Structure):
    _fields_ = [("col0", C.c_int32), ("ncols", C.c_int32), ("dcol0", C.c_int32), ("_pad", C.c_int32)]


class NcwPackDesc(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("g", C.c_void_p), ("bias", C.c_void_p), ("dst_w", C.c_void_p), ("dst_b", C.c_void_p),
        ("ld", C.c_int32), ("row0", C.c_int32), ("nrows", C.c_int32), ("drow0", C.c_int32),
        ("rb_out", C.c_int32), ("rb_in", C.c_int32), ("transpose", C.c_int32), ("prec", C.c_int32),
        ("scale", C.c_float), ("nseg", C.c_int32), ("seg", NcwSeg * MAX_SEGS), ("residual", C.c_int32), ("_pad", C.c_int32),
    ]


class NcwUnpackDesc(C.Structure):
    _fields_ = [
        ("dw", C.c_void_p), ("db", C.c_void_p), ("src", C.c_void_p), ("g", C.c_void_p),
        ("d_src", C.c_void_p), ("d_g", C.c_void_p), ("d_bias", C.c_void_p),
        ("ld", C.c_int32), ("ldw", C.c_int32), ("row0", C.c_int32), ("nrows", C.c_int32), ("drow0", C.c_int32),
        ("scale", C.c_float), ("grad_mul", C.c_float), ("accumulate", C.c_int32), ("nseg", C.c_int32),
        ("seg", NcwSeg * MAX_SEGS), ("grad_mul_dev", C.c_void_p),
    ]


class NcwAdamState(C.Structure):
    _fields_ = [("step", C.c_int32), ("good", C.c_int32), ("skipped", C.c_int32), ("skip_now", C.c_int32),
                ("coef", C.c_float), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("last_norm", C.c_float)]


class NcwSdfNet(C.Structure):
    _fields_ = [
        ("w", C.c_void_p * MAX_LAYERS), ("b", C.c_void_p * MAX_LAYERS), ("wt", C.c_void_p * MAX_LAYERS),
        ("w_feat", C.c_void_p), ("b_feat", C.c_void_p), ("wt_feat", C.c_void_p),
        ("n_layers", C.c_int32), ("skip_layer", C.c_int32), ("rb", C.c_int32), ("multires", C.c_int32),
        ("scale", C.c_float), ("adj_mode", C.c_int32), ("w_lo", C.c_void_p * MAX_LAYERS),
        ("wt_lo", C.c_void_p * MAX_LAYERS),
    ]


class NcwPoints(C.Structure):
    _fields_ = [("x", C.c_void_p), ("rays_o", C.c_void_p), ("rays_d", C.c_void_p), ("z", C.c_void_p),
                ("sample_dist", C.c_void_p), ("per_ray", C.c_int32), ("mode", C.c_int32),
                ("gmin", C.c_float * 3), ("gmax", C.c_float * 3), ("gorigin", C.c_float * 3), ("gradius", C.c_float),
                ("gdim", C.c_int32), ("_gpad", C.c_int32), ("gstart", C.c_int64),
                ("idx", C.c_void_p), ("count", C.c_void_p)]


class NcwNnGrid(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("h", C.c_float), ("inv_h", C.c_float), ("dim", C.c_int32 * 3)]


class NcwPtmGrid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("h", C.c_double), ("inv_h", C.c_double), ("dim", C.c_int32 * 3)]


class NcwRasterView(C.Structure):
    _fields_ = [("view", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("znear", C.c_float), ("zfar", C.c_float), ("height", C.c_int32), ("width", C.c_int32), ("cull", C.c_int32),
                ("small_max", C.c_int32)]


class NcwViewCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("c2w", C.c_float * 12),
                ("width", C.c_int32), ("height", C.c_int32), ("near", C.c_float), ("far", C.c_float)]


class NcwCacheOctree(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("scale", C.c_float), ("level", C.c_int32), ("_pad", C.c_int32),
                ("occ", C.c_void_p), ("brick", C.c_void_p)]


class NcwSourceRec(C.Structure):
    _fields_ = [("pix", C.c_uint32), ("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("label", C.c_uint8)]


class NcwSourceImage(C.Structure):
    _fields_ = [("cam", NcwViewCamera), ("ts", C.c_int32), ("_pad", C.c_int32)]


class NcwVoxelView(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("pose", C.c_float * 9),
                ("o_norm", C.c_float * 3), ("width", C.c_int32), ("height", C.c_int32)]


class NcwPixelQuery(C.Structure):
    _fields_ = [("w2c", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("qx", C.c_float), ("qy", C.c_float)]


class NcwFuseGrid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("h", C.c_double), ("dims", C.c_int64 * 3), ("scale", C.c_double),
                ("off", C.c_double * 3), ("cos_min", C.c_double), ("facing", C.c_int32), ("_pad", C.c_int32)]


class NcwFuseTable(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("acc", C.c_void_p), ("stamp", C.c_void_p), ("views", C.c_void_p),
                ("counters", C.c_void_p), ("capacity", C.c_int64)]


class NcwSynthMaterial(C.Structure):
    _fields_ = [("base", C.c_float * 3), ("freq", C.c_float), ("amp", C.c_float), ("label", C.c_int32)]


class NcwSynthImage(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("c2w", C.c_float * 12),
                ("sfm2gt", C.c_float * 12), ("light", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float),
                ("gain", C.c_float * 3), ("bias", C.c_float * 3), ("sky_top", C.c_float * 3), ("sky_bottom", C.c_float * 3),
                ("height", C.c_int32), ("width", C.c_int32), ("ss", C.c_int32), ("sky_label", C.c_int32), ("tex_seed", C.c_uint32),
                ("_pad", C.c_int32)]


class NcwSynthView(C.Structure):
    _fields_ = [("w2c", C.c_double * 12), ("centre", C.c_double * 3), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("znear", C.c_double), ("sigma_r3", C.c_double), ("depth_tol", C.c_double), ("seed", C.c_uint64),
                ("height", C.c_int32), ("width", C.c_int32), ("serial", C.c_uint32), ("_pad", C.c_int32)]


class NcwDepthMetricsParams(C.Structure):
    _fields_ = [("cam", NcwViewCamera), ("scale", C.c_float), ("delta_thr", C.c_float * 3), ("cos_thr", C.c_float * 3),
                ("n_cos_edges", C.c_int32), ("n_rel_edges", C.c_int32), ("_pad", C.c_int32), ("cos_edges", C.c_void_p),
                ("rel_edges", C.c_void_p)]


DM_PRED_Z, DM_PRED_T = 0, 1    # NCW_DM_PRED_Z / _T: the prediction plane is an eye-space z / trace_view's t
DM_LANES = 256                 # NCW_DM_LANES: lanes of a workgroup of ncw_depthmetrics_view
DM_BLOCK = 2048                # NCW_DM_BLOCK: consecutive pixels of one workgroup
DM_SUMS = 6                    # NCW_DM_SUMS: float64 sums of a row (a, e, ee, r, s, c)
DM_COUNTS = 12                 # NCW_DM_COUNTS: int64 counts of a row
DM_FIXED = 18                  # NCW_DM_FIXED: words of a row in front of the two histograms
DM_MAX_EDGES = 2048            # NCW_DM_MAX_EDGES: most edges of either table
SYNTH_MAX_SS = 4               # NCW_SYNTH_MAX_SS: sub-samples per pixel and axis of ncw_synth_shade
FUSE_ACC = 10                  # NCW_FUSE_ACC: int64 sums per table row (count, qpos [3], qn [3], qc [3])
FUSE_COUNTERS = 4              # NCW_FUSE_COUNTERS: occupied, overflow, valid, spare
FUSE_EMPTY = -1                # NCW_FUSE_EMPTY: the key of a free slot
FUSE_MAX_DIM = 1 << 20         # 2^NCW_FUSE_MAX_DIM_LOG2 cells per axis
FUSE_MAX_CAPACITY = 1 << 36    # 2^NCW_FUSE_MAX_CAPACITY_LOG2 table rows
FUSE_MAX_SERIAL = 0x7ffffffe   # NCW_FUSE_MAX_SERIAL
PIXNN_WG_POINTS = 2048   # NCW_PIXNN_WG_POINTS: consecutive points of one workgroup of ncw_pixel_nearest
PIXNN_QUERY_TILE = 256   # NCW_PIXNN_QUERY_TILE: queries per LDS tile
ALIGN_LANES = 256        # NCW_ALIGN_LANES: lanes of a workgroup of ncw_align_sums
ALIGN_BLOCK = 1024       # NCW_ALIGN_BLOCK: consecutive points of one workgroup
ALIGN_SUMS = 20          # NCW_ALIGN_SUMS: float64 sums of ncw_align_sums


class NcwSdfStash(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("h", C.c_void_p * MAX_LAYERS), ("s", C.c_void_p * MAX_LAYERS),
                ("t", C.c_void_p * MAX_LAYERS), ("feat", C.c_void_p), ("dfeat", C.c_void_p),
                ("qbar", C.c_void_p * MAX_LAYERS), ("zbar", C.c_void_p * MAX_LAYERS), ("zsdf", C.c_void_p),
                ("one", C.c_void_p)]


class NcwWgradDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("dense", C.c_void_p), ("dbias", C.c_void_p),
                ("rbx", C.c_int32), ("rby", C.c_int32), ("ld", C.c_int32), ("ksplit", C.c_int32),
                ("n_points", C.c_int64), ("n_points_dev", C.c_void_p)]


class NcwColorNet(C.Structure):
    _fields_ = [("w_f", C.c_void_p), ("wt_f", C.c_void_p), ("b_f", C.c_void_p),
                ("w_e", C.c_void_p * 4), ("wt_e", C.c_void_p * 4), ("b_e", C.c_void_p * 4),
                ("w_l", C.c_void_p * 8), ("wt_l", C.c_void_p * 8), ("b_l", C.c_void_p * 8),
                ("n_head", C.c_int32), ("n_lin", C.c_int32), ("rbf", C.c_int32), ("rbh", C.c_int32),
                ("rbc", C.c_int32), ("n_a", C.c_int32),
                ("w_f_lo", C.c_void_p), ("w_e_lo", C.c_void_p * 4), ("w_l_lo", C.c_void_p * 8),
                ("act_split", C.c_int32), ("_pad", C.c_int32)]


class NcwColorStash(C.Structure):
    _fields_ = [("aux1", C.c_void_p), ("aux2", C.c_void_p), ("f", C.c_void_p), ("e", C.c_void_p * 4),
                ("x", C.c_void_p * 8), ("zf", C.c_void_p), ("ze", C.c_void_p * 4), ("zx", C.c_void_p * 8),
                ("zo", C.c_void_p), ("aux_bias", C.c_void_p)]


class NcwNerfNet(C.Structure):
    _fields_ = [("w_p", C.c_void_p * 8), ("wt_p", C.c_void_p * 8), ("b_p", C.c_void_p * 8),
                ("w_alpha", C.c_void_p), ("wt_alpha", C.c_void_p), ("b_alpha", C.c_void_p),
                ("w_feat", C.c_void_p), ("wt_feat", C.c_void_p), ("b_feat", C.c_void_p),
                ("w_a", C.c_void_p * 4), ("wt_a", C.c_void_p * 4), ("b_a", C.c_void_p * 4),
                ("w_rgb", C.c_void_p), ("wt_rgb", C.c_void_p), ("b_rgb", C.c_void_p),
                ("D", C.c_int32), ("skip", C.c_int32), ("rbn", C.c_int32), ("rbh", C.c_int32),
                ("n_head", C.c_int32), ("n_a", C.c_int32),
                ("w_p_lo", C.c_void_p * 8), ("w_alpha_lo", C.c_void_p), ("w_feat_lo", C.c_void_p), ("w_a_lo", C.c_void_p * 4),
                ("w_rgb_lo", C.c_void_p)]


class NcwNerfStash(C.Structure):
    _fields_ = [("gp", C.c_void_p), ("aux1", C.c_void_p), ("h", C.c_void_p * 9), ("featn", C.c_void_p),
                ("e", C.c_void_p * 4), ("zp", C.c_void_p * 8), ("zalpha", C.c_void_p), ("zfeat", C.c_void_p),
                ("ze", C.c_void_p * 4), ("zrgb", C.c_void_p), ("aux_bias", C.c_void_p)]


def _ptr_struct(name, fields_ptr, fields_other=()):
    return type(name, (C.Structure,), {"_fields_": [(f, C.c_void_p) for f in fields_ptr] + list(fields_other)})


NcwCompositeIn = _ptr_struct(
    "NcwCompositeIn",
    ["rays_o", "rays_d", "z", "z_feed", "sample_dist", "sdf", "grad", "rgb", "density", "bg_rgb", "inv_s",
     "background_rgb", "cos_anneal_dev"],
    [("cos_anneal", C.c_float), ("R", C.c_int32), ("S", C.c_int32), ("O", C.c_int32), ("has_bg", C.c_int32),
     ("trim_sphere", C.c_int32)],
)
NcwCompositeOut = _ptr_struct(
    "NcwCompositeOut",
    ["color", "color_sphere", "color_bg", "weights", "weights_sum", "cdf", "inside", "depth", "normals", "eik",
     "mid_z", "dists", "bg_alpha", "weights_max"],
)
NcwCompositeGrad = _ptr_struct(
    "NcwCompositeGrad",
    ["d_color", "d_weights_sum", "d_depth", "d_eik_num", "d_sdf", "d_grad", "d_rgb", "d_density", "d_bg_rgb",
     "d_inv_s"],
    [("grad_scale", C.c_float), ("grad_scale_dev", C.c_void_p), ("d_normals", C.c_void_p)],
)

_VP = C.c_void_p
_PROTOS = {
    "ncw_mc_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_mc_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_ray_tail_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_ray_tail_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "ncw_ray_floor_fwd": (C.c_int, [_VP, _VP, _VP, C.c_int, C.POINTER(C.c_float), _VP, _VP, _VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "ncw_ray_floor_bwd": (C.c_int, [_VP, _VP, _VP, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, _VP, _VP, _VP, _VP]),
    "ncw_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p]),
    "ncw_adam_step_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int,
                                    C.c_float, C.c_float, C.c_void_p]),
    "ncw_wgrad_tiled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "ncw_wgrad_tiled_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "ncw_sdf_infer_points": (C.c_int, [C.POINTER(NcwSdfNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p,
                                       C.c_void_p]),
    "ncw_nn_cell_keys": (C.c_int, [_VP, C.c_int64, C.POINTER(NcwNnGrid), _VP, _VP]),
    "ncw_nn_cell_ranges": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "ncw_nn_query": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.POINTER(NcwNnGrid), C.c_int, C.c_float, _VP, _VP, _VP, _VP, _VP]),
    "ncw_nn_brute": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "ncw_nn_coarse": (C.c_int, [_VP, C.POINTER(NcwNnGrid), C.c_int, _VP, _VP]),
    "ncw_nn_query_within": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int64, C.POINTER(NcwNnGrid), C.c_float, C.c_float, _VP, _VP, _VP]),
    "ncw_knn_query": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, _VP, C.c_int64, C.POINTER(NcwNnGrid), C.c_float, C.c_float, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP]),
    "ncw_knn_pca": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float), _VP, _VP, _VP, _VP, _VP]),
    "ncw_imls_values": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(NcwNnGrid), C.c_float, _VP, C.c_int64, C.POINTER(C.c_float), C.c_float,
                                  C.POINTER(C.c_int32), C.c_float, _VP, _VP, _VP, _VP, _VP]),
    "ncw_raster_small": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, C.POINTER(NcwRasterView), _VP, _VP, _VP, _VP]),
    "ncw_raster_large": (C.c_int, [_VP, C.c_int64, _VP, C.POINTER(NcwRasterView), _VP, _VP, C.c_int64, _VP, _VP]),
    "ncw_raster_resolve": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP]),
    "ncw_raster_backproject": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.POINTER(C.c_float), _VP, _VP]),
    "ncw_raster_mark": (C.c_int, [_VP, _VP, C.c_int64, C.c_float, C.c_int64, _VP, _VP]),
    "ncw_view_rays": (C.c_int, [C.POINTER(NcwViewCamera), C.c_int64, C.c_int64, _VP, _VP]),
    "ncw_view_store": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP]),
    "ncw_image_reduce_scratch_bytes": (C.c_int64, []),
    "ncw_image_minmax": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP]),
    "ncw_depth_colormap": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_image_sqerr": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int, _VP, _VP, _VP, _VP]),
    "ncw_image_ssim_scratch_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ncw_image_ssim": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP]),
    "ncw_trace_scratch_bytes": (C.c_int64, [C.c_int64]),
    "ncw_trace_begin": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_trace_step": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, C.c_float, C.c_float, C.c_int, _VP, _VP, _VP,
                                 _VP, _VP, _VP]),
    "ncw_trace_finish": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "ncw_trace_store": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_float), C.c_int64, C.c_int64, C.c_int64,
                                  _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_sfm_depth_splat": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_double, C.POINTER(C.c_float), C.c_int, C.c_int, _VP, _VP, _VP,
                                      _VP]),
    "ncw_cache_rows": (C.c_int, [C.POINTER(NcwViewCamera), _VP, _VP, C.c_int, C.c_int, _VP, _VP, C.c_int, C.c_float,
                                 C.POINTER(NcwCacheOctree), C.POINTER(NcwCacheOctree), C.c_int64, C.c_int64, C.c_int, _VP, _VP,
                                 _VP, _VP]),
    "ncw_source_batch": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, C.c_int, _VP, _VP, _VP, C.POINTER(NcwCacheOctree), C.c_float, _VP,
                                   C.c_int64, C.c_int, _VP, _VP, _VP, _VP, C.POINTER(C.c_int), C.c_int, _VP, _VP]),
    "ncw_surf_weights": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, C.POINTER(C.c_double), _VP, _VP]),
    "ncw_surf_pick": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, _VP, _VP]),
    "ncw_surf_sample": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int, _VP, _VP, _VP,
                                  _VP]),
    "ncw_ptm_pack": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), _VP, _VP, _VP]),
    "ncw_ptm_count": (C.c_int, [_VP, _VP, C.c_int64, C.POINTER(NcwPtmGrid), C.c_int64, _VP, _VP, _VP]),
    "ncw_ptm_emit": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(NcwPtmGrid), C.c_int64, _VP, _VP, _VP]),
    "ncw_ptm_ranges": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int64, _VP, _VP, _VP]),
    "ncw_ptm_cell_keys": (C.c_int, [_VP, C.c_int64, C.POINTER(NcwPtmGrid), _VP, _VP]),
    "ncw_ptm_query": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_int64, C.POINTER(NcwPtmGrid), C.c_int,
                                C.c_double, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_ptm_brute": (C.c_int, [_VP, _VP, C.c_int64, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "ncw_voxel_view_seen": (C.c_int, [C.POINTER(NcwVoxelView), C.POINTER(NcwCacheOctree), C.c_int64, C.c_int64, _VP, _VP, _VP, _VP]),
    "ncw_voxel_points_seen": (C.c_int, [_VP, C.c_int64, C.c_int, _VP, _VP, _VP]),
    "ncw_views_roi": (C.c_int, [_VP, _VP, C.c_int, C.POINTER(C.c_float), C.c_float, _VP, _VP, _VP]),
    "ncw_pixel_nearest": (C.c_int, [_VP, C.c_int, _VP, C.c_int64, C.c_int64, C.c_int, _VP, _VP]),
    "ncw_reproj_errors": (C.c_int, [_VP, C.c_int, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, _VP]),
    "ncw_voxel_build": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_ray_voxel_near_far": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_ray_voxel_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_color_fwd": (C.c_int, [C.POINTER(NcwColorNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcwColorStash), C.c_void_p]),
    "ncw_color_bwd": (C.c_int, [C.POINTER(NcwColorNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcwColorStash),
                                C.c_void_p]),
    "ncw_batch_assemble": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ncw_ray_prologue": (C.c_int, [_VP, C.c_int, C.c_int64, C.POINTER(C.c_float), C.c_float, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_aux_ray_bias": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _VP, _VP, C.c_int, C.c_int64, _VP, C.c_int, _VP]),
    "ncw_inv_s_fwd": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ncw_inv_s_bwd": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP]),
    "ncw_loss_fwd": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_float, C.c_float, C.c_float,
                               C.c_float, _VP, _VP]),
    "ncw_loss_bwd": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                               _VP, _VP, _VP, _VP, _VP]),
    "ncw_scatter_add_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ncw_ray_sum_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ncw_nerf_fwd": (C.c_int, [C.POINTER(NcwNerfNet), C.c_int, C.POINTER(NcwPoints), C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcwNerfStash), C.c_void_p]),
    "ncw_nerf_bwd": (C.c_int, [C.POINTER(NcwNerfNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcwNerfStash), C.c_void_p]),
    "ncw_nerf_refine": (C.c_int, [C.POINTER(NcwNerfNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "ncw_sdf_fwd": (C.c_int, [C.POINTER(NcwSdfNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p, C.c_void_p,
                              C.POINTER(NcwSdfStash), C.c_void_p]),
    "ncw_sdf_bwd": (C.c_int, [C.POINTER(NcwSdfNet), C.c_int, C.POINTER(NcwPoints), C.c_int64, C.c_void_p, C.c_void_p,
                              C.POINTER(NcwSdfStash), C.c_void_p]),
    "ncw_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "ncw_wgrad_ordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                    C.c_void_p]),
    "ncw_wgrad_ordered_scratch_floats": (C.c_int64, [C.c_int]),
    "ncw_stash_from_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ncw_stash_to_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ncw_sdf_infer_rays": (C.c_int, [C.POINTER(NcwSdfNet), C.c_int, _VP, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "ncw_sample_coarse": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ncw_upsample": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_float, C.c_int, _VP, _VP]),
    "ncw_sort_merge": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, _VP]),
    "ncw_boundary": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _VP, _VP]),
    "ncw_bg_select": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, _VP]),
    "ncw_composite_fwd": (C.c_int, [C.POINTER(NcwCompositeIn), C.POINTER(NcwCompositeOut), _VP]),
    "ncw_composite_bwd": (C.c_int, [C.POINTER(NcwCompositeIn), C.POINTER(NcwCompositeGrad), _VP]),
    "ncw_appfit_loss": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_float, _VP, _VP, _VP, _VP, _VP,
                                  _VP]),
    "ncw_appfit_step_scratch_floats": (C.c_int64, [C.c_int64, C.c_int]),
    "ncw_appfit_step": (C.c_int, [_VP, C.c_int64, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP, _VP, _VP, C.c_float, C.c_float,
                                  C.c_float, C.c_float, _VP, C.c_float, _VP, C.c_int64, _VP]),
    "ncw_mesh_cc_hook": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, _VP]),
    "ncw_mesh_cc_flatten": (C.c_int, [_VP, C.c_int64, _VP]),
    "ncw_mesh_cc_sizes": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, _VP, _VP]),
    "ncw_mesh_face_select": (C.c_int, [_VP, C.c_int64, C.c_int64, _VP, C.c_int, _VP, _VP, _VP, _VP]),
    "ncw_mesh_compact_mark": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, _VP]),
    "ncw_mesh_compact_faces": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int64, C.c_int64, _VP, _VP]),
    "ncw_mesh_sc_keys": (C.c_int, [_VP, _VP, C.c_int64, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64), _VP, _VP]),
    "ncw_mesh_sc_faces": (C.c_int, [_VP, C.c_int64, C.c_int64, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "ncw_mesh_sc_place": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, _VP, _VP, C.c_int64, _VP, _VP, C.c_int64,
                                    C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64), C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "ncw_align_transform": (C.c_int, [_VP, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.c_float, _VP, _VP, _VP]),
    "ncw_align_sums_blocks": (C.c_int64, [C.c_int64]),
    "ncw_align_sums": (C.c_int, [_VP, C.c_int64, C.POINTER(C.c_double), _VP, C.c_int64, C.POINTER(C.c_double), _VP, _VP, C.c_float,
                                 C.POINTER(C.c_double), _VP, _VP, _VP, _VP, _VP]),
    "ncw_mcs_neighbors": (C.c_int, [_VP, C.c_int64, C.c_int, _VP, _VP]),
    "ncw_mcs_count": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int, C.c_int, C.c_float, _VP, _VP, _VP]),
    "ncw_mcs_cube_ids": (C.c_int, [_VP, C.c_int64, C.c_int, C.c_int, _VP, C.c_int64, _VP, _VP]),
    "ncw_mcs_emit": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int, C.c_int, C.c_float, _VP, _VP, _VP, _VP, _VP, C.c_int64,
                               C.c_int64, _VP, _VP, _VP]),
    "ncw_fuse_insert": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.POINTER(NcwFuseGrid), C.POINTER(NcwFuseTable), _VP]),
    "ncw_fuse_move": (C.c_int, [C.POINTER(NcwFuseTable), C.POINTER(NcwFuseTable), _VP]),
    "ncw_fuse_resolve": (C.c_int, [C.POINTER(NcwFuseTable), _VP, C.c_int64, C.POINTER(NcwFuseGrid), _VP, _VP, _VP, _VP, _VP, _VP,
                                   _VP, _VP]),
    "ncw_synth_shade": (C.c_int, [_VP, _VP, C.POINTER(NcwSynthImage), _VP, _VP, C.c_int64, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "ncw_synth_observe": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(NcwSynthView), _VP, _VP, _VP, _VP, _VP]),
    "ncw_depthmetrics_scratch_bytes": (C.c_int64, [C.c_int64]),
    "ncw_depthmetrics_view": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(NcwDepthMetricsParams), _VP, _VP,
                                        C.c_int64, C.c_int64, _VP, _VP, _VP, _VP]),
    "ncw_abi_version": (C.c_int, []),
    "ncw_source_hash": (C.c_char_p, []),
    "ncw_device_info": (C.c_int, [C.c_char_p, C.c_int]),
    "ncw_grad_norm_scratch_floats": (C.c_int64, []),
    "ncw_grad_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ncw_pack_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ncw_unpack_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ncw_sdf_infer": (C.c_int, [C.POINTER(NcwSdfNet), C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

_lib = None

# Optional per-entry-point HIP-event timing (bench.py's roofline leg): when PROFILE is a dict, every
# C-ABI call is bracketed by events recorded on torch's current stream (the stream the kernel is
# launched on) and appended to PROFILE[name].
PROFILE = None


def _wrap_timed(name, fn):
    def call(*args):
        if PROFILE is None:
            return fn(*args)
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*args)
        e1.record()
        PROFILE.setdefault(name, []).append((e0, e1))
        return r

    return call



class NeuconwHipError(RuntimeError):
    pass


def exported_symbols():
    """Names every entry point include/neuconw_hip.h declares (used by the CPU-side ABI test)."""
    return sorted(_PROTOS)


def get_lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NeuconwHipError(
            "libneuconw_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no CPU / PyTorch fallback for the hot path." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    ns = type("NcwLib", (), {})()
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale: fail loudly
        fn.restype = res
        fn.argtypes = args
        setattr(ns, name, _wrap_timed(name, fn))
    v = lib.ncw_abi_version()
    if v != ABI_VERSION:
        raise NeuconwHipError("libneuconw_hip.so ABI %d != binding ABI %d: rebuild" % (v, ABI_VERSION))
    # the library must have been built from the sources in this tree (build.source_hash): a stale prebuilt .so -- e.g. one
    # shipped to a GPU box after csrc/ changed -- is refused, not silently tested.  Probe variants (NEUCONW_HIP_LIB) are exempt.
    if not os.environ.get("NEUCONW_HIP_LIB") and os.path.isdir(os.path.join(HERE, "csrc")):
        from . import build as _b

        built, now = lib.ncw_source_hash().decode(), _b.source_hash()
        if built != now:
            raise NeuconwHipError("libneuconw_hip.so was built from other sources (%s.. != %s..): rebuild with "
                                  "`python -c 'import __graft_entry__ as g; g.build()'`" % (built[:12], now[:12]))
    ns._cdll = lib
    _lib = ns
    return ns


def check(code, what):
    if code != 0:
        raise NeuconwHipError("%s failed with code %d" % (what, code))


def stream_ptr(device=None):
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device pointer of a contiguous torch tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "non-contiguous tensor handed to the C ABI"
    return C.c_void_p(t.data_ptr())
