"""GPU: `ncw_sdf_bwd` -- the first- and second-order backward of the SDF network -- at its depths, skip positions and cotangent parts:
sdf_bwd_kernel (csrc/ncw_sdf.hip: W = 64 / 256 in every precision, W = 512 at n_lin = 2), sdf_bwd16_kernel<T> (csrc/ncw_sdf16.hip:
W = 512, 16-bit, T = 2 / 3 / 4 tiles per workgroup) and sdf_bwd16f_kernel (csrc/ncw_sdf16f.hip: W = 512, fp32).  The reference is
tests/_sdf_bwd_ref.py (checked on the CPU by tests/test_sdf_bwd_ref_host.py): an fp64 statement of every field the backward stores.

a. EXACT: a column of an MFMA depends on nothing but its own point, so forward + backward of the same points in another launch
   decomposition give the same bits in every stash field and output.  At W = 512 a child process re-runs the 16-bit cases with
   NCW_SDF16_T = 3 and 4 (the small launches here pick T = 2 on their own).
b. EXACT: the backward writes what it owns -- the arena is filled with NaN bit patterns before the forward, so a read of anything
   no kernel wrote shows; gamma, h, s, t, feat and dfeat keep their bytes over all allocated tiles; d_grad = 0 leaves every qbar row
   zero (pass 1 then parks zeros: zbar2 contributes nothing and zbar stays finite); d_sdf = 0 leaves zsdf zero; `one` is 1 for the
   valid points and 0 for the padded lanes and every other feature of its block.
c. EXACT: ray-indexed points (NcwPoints mode 1 / 2) whose generation is exact in fp32 equal the mode-0 run on the same points, every
   field; mode 4, a bad precision and n = 0 return before any launch.
d. Against the fp64 statement, separately for the first-order part (d_grad = 0), the second-order part (d_sdf = 0, d_feat = 0) and
   both: every per-point field and every parameter gradient (add_wgrads / unpack_grads against torch.autograd.grad of
   oracle.sdf_net), tests/_util.rel_err.  tests/test_gpu_sdf_train.py cannot see the first-order part: it is 2 % - 18 % of the max
   norm of a field under `both`, less than the bf16 bound there.
e. What part d found on its first run: the cache key of PackPlan.unpack_grads (test_unpack_table_is_keyed_by_every_gradient_tensor).

Bounds of d. -- none comes from the kernels.  Per-point fields: 2 x the 16-bit rounding floor (bf16 / f16), max(2e-4, 2 x the fp32
floor) (f32).  Parameter gradients: (8, (4,)) takes the bounds of tests/test_gpu_sdf_train.py as they are (f32 2e-4; 16-bit under
`both`: bf16 0.25, f16 0.03 at W = 64 and 8e-3 above); every other shape (the one with scale = 1.7 too) or cotangent set max(that bound, 2 x floor), per parameter.
The floors are those of tests/_sdf_bwd_ref.py: the same statement with each unavoidable 16-bit rounding made once (listed there), or
evaluated by torch in fp32.  The factor 2 is the margin of tests/test_gpu_color_edges.py for the same construction: f32 accumulation
order, the fast exp and ties, each at least 2^-13 below a 16-bit rounding.  A field whose reference is identically zero must be zero.

Which branch of the weight-prefetch chain a network takes (L = n_layers + 1; the three kernels share the structure: pass 1 walks
w[0] .. w[L-2] and prefetches wt_feat last; pass 2 multiplies wt_feat and wt[L-1], then wt[L-2] .. wt[1], each prefetched a layer
ahead; FCB_* = the first-chunk size of sdf_bwd_kernel's ring, 16 / 18 = the out-block stride of the W = 512 kernels' prefetch):
  (8, (4,))   L = 9, skip 4: pass 1 prefetches a hidden matrix (FCB_WH) except in front of l = 4 (FCB_WS, K = W + 39 with the gamma
              units); pass 2 prefetches wt[4] as the skip transpose (FCB_TS / 18 blocks) while wt[5] runs, the others FCB_WH / 16.
  (1, ())     L = 2: both loops run once; pass 1's only prefetch is wt_feat, pass 2 has no next matrix at all (`nullptr`: m = 0).  At
              W = 512 this is the only network on sdf_bwd_kernel<., 16> (the streamed kernels need L >= 3).
  (2, (1,))   L = 3, skip = L-2 = 1: pass 1 prefetches the skip matrix first (FCB_WS) and wt_feat behind it; the FIRST prefetch of
              pass 2 (issued with the wt[L-1] product) is the skip transpose (FCB_TS / 18 blocks), and it is the last (wt[0] is never
              multiplied: nothing consumes u_0).
  (3, (1,))   L = 4, skip 1: `l + 1 == skip` at l = 0 in pass 1; in pass 2 the skip transpose is prefetched INSIDE the loop (while
              wt[2] runs, `l - 1 == skip`) and consumed as the last product.
  (3, ())     L = 4, no skip: no gamma job, no FCB_WS / FCB_TS, every prefetch FCB_WH / 16.
  (11, (10,)) L = 12 = NCW_MAX_LAYERS, skip = L-2 = 10: the last slot of every struct array is live; as (2, (1,)) the first prefetch
              of pass 2 is the skip transpose, followed by nine plain ones.

Measured on MI355X (printed by part d: per case the per-point field and the parameter gradient closest to their bounds):
  W256-n8s4         f32  first   field zbar7  gpu 3.38e-06 floor 2.99e-06   gradient lin6.bias        gpu 1.55e-06 floor 6.29e-07 bound 2.00e-04
  W256-n8s4         f32  second  field zbar7  gpu 3.95e-06 floor 2.79e-06   gradient lin7.weight_v    gpu 3.68e-06 floor 2.53e-06 bound 2.00e-04
  W256-n8s4         f32  both    field zbar5  gpu 3.95e-06 floor 3.11e-06   gradient lin7.weight_v    gpu 4.10e-06 floor 2.44e-06 bound 2.00e-04
  W256-n8s4         bf16 first   field zbar3  gpu 1.89e-02 floor 1.87e-02   gradient lin0.weight_v    gpu 1.04e-02 floor 9.97e-03 bound 2.50e-01
  W256-n8s4         bf16 second  field zbar5  gpu 2.84e-02 floor 2.67e-02   gradient lin8.weight_g    gpu 3.96e-02 floor 4.11e-02 bound 2.50e-01
  W256-n8s4         bf16 both    field zbar5  gpu 2.89e-02 floor 2.72e-02   gradient lin7.weight_v    gpu 2.67e-02 floor 2.56e-02 bound 2.50e-01
  W256-n8s4         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin5.weight_g    gpu 7.11e-04 floor 5.55e-04 bound 8.00e-03
  W256-n8s4         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin8.weight_g    gpu 2.72e-03 floor 2.66e-04 bound 8.00e-03
  W256-n8s4         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.weight_g    gpu 1.35e-03 floor 3.39e-03 bound 8.00e-03
  W256-n1sx         f32  first   field zbar0  gpu 6.51e-07 floor 8.73e-07   gradient lin1.weight_v    gpu 5.27e-07 floor 8.26e-07 bound 2.00e-04
  W256-n1sx         f32  second  field zbar0  gpu 1.05e-06 floor 7.07e-07   gradient lin0.weight_g    gpu 3.97e-07 floor 7.01e-07 bound 2.00e-04
  W256-n1sx         f32  both    field zbar0  gpu 1.03e-06 floor 7.15e-07   gradient lin0.bias        gpu 3.84e-07 floor 4.11e-07 bound 2.00e-04
  W256-n1sx         bf16 first   field zbar0  gpu 1.63e-02 floor 1.31e-02   gradient lin0.weight_v    gpu 5.13e-03 floor 4.67e-03 bound 2.50e-01
  W256-n1sx         bf16 second  field qbar0  gpu 2.78e-03 floor 2.78e-03   gradient lin0.bias        gpu 1.05e-02 floor 1.09e-02 bound 2.50e-01
  W256-n1sx         bf16 both    field zbar0  gpu 1.88e-02 floor 1.73e-02   gradient lin0.bias        gpu 9.97e-03 floor 9.22e-03 bound 2.50e-01
  W256-n1sx         f16  first   field zbar0  gpu 2.65e-03 floor 2.28e-03   gradient lin1.weight_v    gpu 5.54e-04 floor 5.52e-04 bound 8.00e-03
  W256-n1sx         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin0.bias        gpu 1.94e-03 floor 1.92e-03 bound 8.00e-03
  W256-n1sx         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 1.88e-03 floor 2.06e-03 bound 8.00e-03
  W256-n2s1         f32  first   field zbar1  gpu 2.14e-06 floor 1.28e-06   gradient lin2.weight_v    gpu 5.56e-07 floor 7.58e-07 bound 2.00e-04
  W256-n2s1         f32  second  field zbar1  gpu 1.59e-06 floor 1.75e-06   gradient lin2.weight_g    gpu 1.16e-06 floor 1.04e-06 bound 2.00e-04
  W256-n2s1         f32  both    field zbar1  gpu 1.58e-06 floor 1.75e-06   gradient lin2.weight_g    gpu 8.38e-07 floor 4.92e-07 bound 2.00e-04
  W256-n2s1         bf16 first   field zbar1  gpu 1.61e-02 floor 1.33e-02   gradient lin2.weight_v    gpu 5.45e-03 floor 5.45e-03 bound 2.50e-01
  W256-n2s1         bf16 second  field qbar0  gpu 2.78e-03 floor 2.78e-03   gradient lin1.bias        gpu 1.14e-02 floor 1.25e-02 bound 2.50e-01
  W256-n2s1         bf16 both    field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin1.bias        gpu 1.10e-02 floor 1.20e-02 bound 2.50e-01
  W256-n2s1         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin1.weight_g    gpu 6.61e-04 floor 6.04e-04 bound 8.00e-03
  W256-n2s1         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin1.bias        gpu 4.87e-04 floor 1.40e-03 bound 8.00e-03
  W256-n2s1         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.weight_g    gpu 6.46e-04 floor 1.37e-03 bound 8.00e-03
  W256-n3s1         f32  first   field zbar2  gpu 2.52e-06 floor 2.65e-06   gradient lin1.weight_v    gpu 5.98e-07 floor 3.73e-07 bound 2.00e-04
  W256-n3s1         f32  second  field zbar2  gpu 2.80e-06 floor 2.67e-06   gradient lin2.weight_v    gpu 2.49e-06 floor 2.14e-06 bound 2.00e-04
  W256-n3s1         f32  both    field zbar2  gpu 2.80e-06 floor 2.68e-06   gradient lin2.weight_v    gpu 2.54e-06 floor 2.44e-06 bound 2.00e-04
  W256-n3s1         bf16 first   field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.weight_g    gpu 7.77e-03 floor 8.16e-03 bound 2.50e-01
  W256-n3s1         bf16 second  field zbar2  gpu 3.25e-02 floor 2.77e-02   gradient lin1.bias        gpu 2.52e-02 floor 2.42e-02 bound 2.50e-01
  W256-n3s1         bf16 both    field zbar2  gpu 3.29e-02 floor 2.85e-02   gradient lin1.bias        gpu 2.56e-02 floor 2.83e-02 bound 2.50e-01
  W256-n3s1         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.weight_v    gpu 6.05e-04 floor 7.70e-04 bound 8.00e-03
  W256-n3s1         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin0.weight_g    gpu 7.81e-04 floor 1.77e-03 bound 8.00e-03
  W256-n3s1         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.bias        gpu 8.82e-04 floor 2.14e-03 bound 8.00e-03
  W256-n3sx         f32  first   field zbar2  gpu 2.42e-06 floor 2.12e-06   gradient lin0.weight_v    gpu 6.91e-07 floor 5.25e-07 bound 2.00e-04
  W256-n3sx         f32  second  field zbar2  gpu 4.03e-06 floor 2.45e-06   gradient lin2.weight_v    gpu 2.39e-06 floor 1.14e-06 bound 2.00e-04
  W256-n3sx         f32  both    field zbar2  gpu 4.01e-06 floor 2.43e-06   gradient lin2.weight_v    gpu 2.31e-06 floor 1.12e-06 bound 2.00e-04
  W256-n3sx         bf16 first   field zbar1  gpu 6.25e-03 floor 6.05e-03   gradient lin2.bias        gpu 8.72e-03 floor 8.24e-03 bound 2.50e-01
  W256-n3sx         bf16 second  field zbar2  gpu 3.36e-02 floor 3.16e-02   gradient lin1.bias        gpu 1.51e-02 floor 1.42e-02 bound 2.50e-01
  W256-n3sx         bf16 both    field zbar2  gpu 3.40e-02 floor 3.20e-02   gradient lin3.weight_g    gpu 2.72e-02 floor 2.73e-02 bound 2.50e-01
  W256-n3sx         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin3.weight_v    gpu 7.01e-04 floor 1.20e-03 bound 8.00e-03
  W256-n3sx         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin2.bias        gpu 6.49e-04 floor 2.38e-03 bound 8.00e-03
  W256-n3sx         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.bias        gpu 6.31e-04 floor 2.47e-03 bound 8.00e-03
  W256-n11s10       f32  first   field zbar10 gpu 3.20e-06 floor 2.98e-06   gradient lin6.weight_g    gpu 2.00e-06 floor 6.50e-07 bound 2.00e-04
  W256-n11s10       f32  second  field zbar9  gpu 8.65e-06 floor 5.18e-06   gradient lin4.bias        gpu 5.72e-06 floor 3.37e-06 bound 2.00e-04
  W256-n11s10       f32  both    field zbar9  gpu 8.62e-06 floor 5.05e-06   gradient lin4.bias        gpu 5.22e-06 floor 3.02e-06 bound 2.00e-04
  W256-n11s10       bf16 first   field zbar9  gpu 2.10e-02 floor 1.84e-02   gradient lin1.weight_v    gpu 1.41e-02 floor 1.26e-02 bound 2.50e-01
  W256-n11s10       bf16 second  field zbar3  gpu 3.20e-02 floor 2.52e-02   gradient lin3.weight_g    gpu 5.13e-02 floor 4.88e-02 bound 2.50e-01
  W256-n11s10       bf16 both    field zbar3  gpu 3.07e-02 floor 2.39e-02   gradient lin7.weight_v    gpu 5.19e-02 floor 6.12e-02 bound 2.50e-01
  W256-n11s10       f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin11.weight_v   gpu 8.72e-04 floor 6.43e-04 bound 8.00e-03
  W256-n11s10       f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin4.bias        gpu 1.39e-03 floor 4.38e-03 bound 8.76e-03
  W256-n11s10       f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin4.bias        gpu 1.86e-03 floor 4.14e-03 bound 8.28e-03
  W512-n8s4         f32  first   field zbar7  gpu 4.65e-06 floor 2.43e-06   gradient lin6.weight_v    gpu 2.05e-06 floor 9.62e-07 bound 2.00e-04
  W512-n8s4         f32  second  field zbar3  gpu 4.13e-06 floor 2.01e-06   gradient lin7.bias        gpu 3.63e-06 floor 1.50e-06 bound 2.00e-04
  W512-n8s4         f32  both    field zbar3  gpu 4.18e-06 floor 2.04e-06   gradient lin7.bias        gpu 3.51e-06 floor 1.45e-06 bound 2.00e-04
  W512-n8s4         bf16 first   field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin3.bias        gpu 1.56e-02 floor 2.05e-02 bound 2.50e-01
  W512-n8s4         bf16 second  field zbar1  gpu 1.84e-02 floor 1.58e-02   gradient lin2.weight_g    gpu 2.19e-02 floor 1.96e-02 bound 2.50e-01
  W512-n8s4         bf16 both    field zbar5  gpu 1.99e-02 floor 1.98e-02   gradient lin7.weight_v    gpu 2.01e-02 floor 1.98e-02 bound 2.50e-01
  W512-n8s4         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 1.02e-03 floor 1.14e-03 bound 8.00e-03
  W512-n8s4         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin5.weight_g    gpu 1.22e-03 floor 2.79e-03 bound 8.00e-03
  W512-n8s4         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin8.weight_g    gpu 1.82e-03 floor 9.22e-05 bound 8.00e-03
  W512-n1sx         f32  first   field zbar0  gpu 8.53e-07 floor 5.62e-07   gradient lin0.bias        gpu 6.10e-07 floor 4.10e-07 bound 2.00e-04
  W512-n1sx         f32  second  field zbar0  gpu 7.30e-07 floor 7.11e-07   gradient lin1.weight_v    gpu 4.24e-07 floor 9.07e-07 bound 2.00e-04
  W512-n1sx         f32  both    field zbar0  gpu 7.48e-07 floor 7.21e-07   gradient lin1.weight_v    gpu 4.39e-07 floor 9.08e-07 bound 2.00e-04
  W512-n1sx         bf16 first   field zbar0  gpu 1.12e-02 floor 9.50e-03   gradient lin0.bias        gpu 6.43e-03 floor 5.93e-03 bound 2.50e-01
  W512-n1sx         bf16 second  field qbar0  gpu 2.78e-03 floor 2.78e-03   gradient lin0.bias        gpu 6.88e-03 floor 7.77e-03 bound 2.50e-01
  W512-n1sx         bf16 both    field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.bias        gpu 6.84e-03 floor 7.26e-03 bound 2.50e-01
  W512-n1sx         f16  first   field zbar0  gpu 1.44e-03 floor 1.41e-03   gradient lin0.bias        gpu 6.42e-04 floor 6.65e-04 bound 8.00e-03
  W512-n1sx         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin1.weight_g    gpu 1.49e-03 floor 1.66e-03 bound 8.00e-03
  W512-n1sx         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 9.47e-04 floor 1.00e-03 bound 8.00e-03
  W512-n2s1         f32  first   field zbar1  gpu 1.67e-06 floor 8.66e-07   gradient lin0.bias        gpu 7.76e-07 floor 6.31e-07 bound 2.00e-04
  W512-n2s1         f32  second  field zbar1  gpu 2.06e-06 floor 1.25e-06   gradient lin2.weight_g    gpu 7.02e-05 floor 3.60e-05 bound 2.00e-04
  W512-n2s1         f32  both    field zbar1  gpu 2.05e-06 floor 1.25e-06   gradient lin1.bias        gpu 9.10e-07 floor 5.48e-07 bound 2.00e-04
  W512-n2s1         bf16 first   field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.bias        gpu 6.32e-03 floor 6.47e-03 bound 2.50e-01
  W512-n2s1         bf16 second  field qbar0  gpu 2.78e-03 floor 2.78e-03   gradient lin2.weight_g    gpu 1.00e+00 floor 1.01e+00 bound 2.01e+00
  W512-n2s1         bf16 both    field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.bias        gpu 1.36e-02 floor 1.35e-02 bound 2.50e-01
  W512-n2s1         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.weight_v    gpu 5.15e-04 floor 4.83e-04 bound 8.00e-03
  W512-n2s1         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin2.weight_g    gpu 7.75e-02 floor 2.53e-01 bound 5.05e-01
  W512-n2s1         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 5.76e-04 floor 1.25e-03 bound 8.00e-03
  W512-n3s1         f32  first   field zbar2  gpu 2.33e-06 floor 1.71e-06   gradient lin1.bias        gpu 1.09e-06 floor 5.37e-07 bound 2.00e-04
  W512-n3s1         f32  second  field zbar2  gpu 2.64e-06 floor 2.52e-06   gradient lin2.weight_v    gpu 1.56e-06 floor 1.08e-06 bound 2.00e-04
  W512-n3s1         f32  both    field zbar2  gpu 2.64e-06 floor 2.52e-06   gradient lin3.weight_g    gpu 4.46e-06 floor 2.04e-06 bound 2.00e-04
  W512-n3s1         bf16 first   field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.weight_g    gpu 8.51e-03 floor 6.68e-03 bound 2.50e-01
  W512-n3s1         bf16 second  field qbar0  gpu 2.78e-03 floor 2.78e-03   gradient lin2.bias        gpu 1.25e-02 floor 1.17e-02 bound 2.50e-01
  W512-n3s1         bf16 both    field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin3.weight_g    gpu 1.97e-02 floor 2.01e-02 bound 2.50e-01
  W512-n3s1         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.weight_v    gpu 7.16e-04 floor 9.79e-04 bound 8.00e-03
  W512-n3s1         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin1.bias        gpu 8.91e-04 floor 1.13e-03 bound 8.00e-03
  W512-n3s1         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin3.weight_g    gpu 3.59e-03 floor 1.25e-03 bound 8.00e-03
  W512-n3sx         f32  first   field zbar2  gpu 2.22e-06 floor 1.58e-06   gradient lin2.weight_v    gpu 1.42e-06 floor 8.29e-07 bound 2.00e-04
  W512-n3sx         f32  second  field zbar2  gpu 3.34e-06 floor 2.03e-06   gradient lin2.bias        gpu 1.73e-06 floor 1.09e-06 bound 2.00e-04
  W512-n3sx         f32  both    field zbar2  gpu 3.40e-06 floor 1.99e-06   gradient lin2.bias        gpu 1.69e-06 floor 1.10e-06 bound 2.00e-04
  W512-n3sx         bf16 first   field zbar2  gpu 1.67e-02 floor 1.55e-02   gradient lin2.weight_v    gpu 9.08e-03 floor 9.00e-03 bound 2.50e-01
  W512-n3sx         bf16 second  field zbar2  gpu 3.28e-02 floor 2.86e-02   gradient lin2.weight_v    gpu 1.41e-02 floor 1.35e-02 bound 2.50e-01
  W512-n3sx         bf16 both    field zbar2  gpu 3.39e-02 floor 2.96e-02   gradient lin2.bias        gpu 1.35e-02 floor 1.37e-02 bound 2.50e-01
  W512-n3sx         f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin3.weight_v    gpu 1.09e-03 floor 6.36e-04 bound 8.00e-03
  W512-n3sx         f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin2.bias        gpu 7.18e-04 floor 1.85e-03 bound 8.00e-03
  W512-n3sx         f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin2.bias        gpu 7.31e-04 floor 1.78e-03 bound 8.00e-03
  W512-n11s10       f32  first   field zbar10 gpu 3.65e-06 floor 2.61e-06   gradient lin2.weight_g    gpu 3.13e-06 floor 1.80e-06 bound 2.00e-04
  W512-n11s10       f32  second  field zbar10 gpu 7.67e-06 floor 2.74e-06   gradient lin7.weight_g    gpu 5.86e-06 floor 3.22e-06 bound 2.00e-04
  W512-n11s10       f32  both    field zbar10 gpu 7.61e-06 floor 2.76e-06   gradient lin7.weight_g    gpu 5.77e-06 floor 3.12e-06 bound 2.00e-04
  W512-n11s10       bf16 first   field zbar6  gpu 1.89e-02 floor 1.38e-02   gradient lin9.weight_g    gpu 2.20e-02 floor 8.71e-03 bound 2.50e-01
  W512-n11s10       bf16 second  field zbar2  gpu 2.67e-02 floor 2.39e-02   gradient lin5.weight_v    gpu 3.31e-02 floor 3.23e-02 bound 2.50e-01
  W512-n11s10       bf16 both    field zbar2  gpu 2.69e-02 floor 2.40e-02   gradient lin9.weight_v    gpu 3.34e-02 floor 3.53e-02 bound 2.50e-01
  W512-n11s10       f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin9.weight_g    gpu 1.23e-03 floor 1.36e-03 bound 8.00e-03
  W512-n11s10       f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin8.weight_g    gpu 1.57e-03 floor 2.44e-03 bound 8.00e-03
  W512-n11s10       f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin4.weight_v    gpu 1.45e-03 floor 3.27e-03 bound 8.00e-03
  W64-n8s4          f32  first   field zbar7  gpu 2.22e-06 floor 2.10e-06   gradient lin3.weight_v    gpu 2.69e-06 floor 1.26e-06 bound 2.00e-04
  W64-n8s4          f32  second  field zbar3  gpu 6.97e-06 floor 5.01e-06   gradient lin2.weight_g    gpu 4.99e-06 floor 4.13e-06 bound 2.00e-04
  W64-n8s4          f32  both    field zbar3  gpu 6.95e-06 floor 4.99e-06   gradient lin2.weight_g    gpu 4.53e-06 floor 4.49e-06 bound 2.00e-04
  W64-n8s4          bf16 first   field zbar7  gpu 4.34e-02 floor 4.25e-02   gradient lin2.weight_g    gpu 5.20e-02 floor 5.20e-02 bound 2.50e-01
  W64-n8s4          bf16 second  field zbar4  gpu 3.01e-02 floor 2.96e-02   gradient lin3.weight_g    gpu 9.82e-02 floor 9.78e-02 bound 2.50e-01
  W64-n8s4          bf16 both    field zbar4  gpu 3.01e-02 floor 2.96e-02   gradient lin3.weight_g    gpu 1.21e-01 floor 1.03e-01 bound 2.50e-01
  W64-n8s4          f16  first   field zbar5  gpu 2.13e-03 floor 2.00e-03   gradient lin0.weight_g    gpu 2.97e-03 floor 2.86e-03 bound 3.00e-02
  W64-n8s4          f16  second  field zbar7  gpu 5.77e-03 floor 5.35e-03   gradient lin3.weight_g    gpu 1.27e-02 floor 1.32e-02 bound 3.00e-02
  W64-n8s4          f16  both    field zbar7  gpu 5.70e-03 floor 5.30e-03   gradient lin3.weight_g    gpu 1.34e-02 floor 1.45e-02 bound 3.00e-02
  W64-n1sx          f32  first   field zbar0  gpu 5.08e-07 floor 4.31e-07   gradient lin0.weight_g    gpu 4.95e-07 floor 4.77e-07 bound 2.00e-04
  W64-n1sx          f32  second  field zbar0  gpu 1.53e-06 floor 8.17e-07   gradient lin0.bias        gpu 4.15e-07 floor 4.05e-07 bound 2.00e-04
  W64-n1sx          f32  both    field zbar0  gpu 1.54e-06 floor 8.13e-07   gradient lin0.bias        gpu 4.57e-07 floor 4.77e-07 bound 2.00e-04
  W64-n1sx          bf16 first   field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.bias        gpu 4.28e-03 floor 4.49e-03 bound 2.50e-01
  W64-n1sx          bf16 second  field zbar0  gpu 3.43e-02 floor 3.40e-02   gradient lin0.bias        gpu 1.40e-02 floor 1.52e-02 bound 2.50e-01
  W64-n1sx          bf16 both    field zsdf   gpu 2.18e-03 floor 2.18e-03   gradient lin0.bias        gpu 1.43e-02 floor 1.70e-02 bound 2.50e-01
  W64-n1sx          f16  first   field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 7.79e-04 floor 7.45e-04 bound 3.00e-02
  W64-n1sx          f16  second  field qbar0  gpu 2.34e-04 floor 2.34e-04   gradient lin0.bias        gpu 1.49e-03 floor 1.53e-03 bound 3.00e-02
  W64-n1sx          f16  both    field zsdf   gpu 2.65e-04 floor 2.65e-04   gradient lin0.bias        gpu 1.54e-03 floor 1.60e-03 bound 3.00e-02
  W64-n8s4-scale1.7 f32  first   field zbar7  gpu 5.94e-06 floor 4.01e-06   gradient lin6.weight_g    gpu 2.08e-06 floor 1.86e-06 bound 2.00e-04
  W64-n8s4-scale1.7 f32  second  field zbar5  gpu 8.21e-06 floor 7.00e-06   gradient lin4.weight_g    gpu 6.83e-06 floor 4.83e-06 bound 2.00e-04
  W64-n8s4-scale1.7 f32  both    field zbar5  gpu 8.25e-06 floor 7.04e-06   gradient lin4.weight_g    gpu 6.93e-06 floor 5.49e-06 bound 2.00e-04
  W64-n8s4-scale1.7 bf16 first   field zbar0  gpu 3.17e-02 floor 2.80e-02   gradient lin6.bias        gpu 2.96e-02 floor 3.24e-02 bound 2.50e-01
  W64-n8s4-scale1.7 bf16 second  field zbar0  gpu 8.19e-02 floor 7.99e-02   gradient lin3.weight_g    gpu 1.24e-01 floor 1.22e-01 bound 2.50e-01
  W64-n8s4-scale1.7 bf16 both    field zbar2  gpu 5.48e-02 floor 5.41e-02   gradient lin3.weight_g    gpu 1.24e-01 floor 1.25e-01 bound 2.51e-01
  W64-n8s4-scale1.7 f16  first   field zbar5  gpu 3.93e-03 floor 3.34e-03   gradient lin0.weight_g    gpu 3.84e-03 floor 4.16e-03 bound 3.00e-02
  W64-n8s4-scale1.7 f16  second  field zbar4  gpu 7.12e-03 floor 6.57e-03   gradient lin6.weight_v    gpu 1.63e-02 floor 1.60e-02 bound 3.20e-02
  W64-n8s4-scale1.7 f16  both    field zbar4  gpu 7.14e-03 floor 6.60e-03   gradient lin6.weight_v    gpu 1.59e-02 floor 1.56e-02 bound 3.12e-02
The floors of the last Linear's weight_g under `second` at (2, (1,)) are large (W = 512: f32 3.6e-5, f16 0.25, bf16 1.0): the geometric
initialisation makes that row nearly parallel to its gradient, and weight-norm's projection cancels; the statement says so itself.
Wall time of the file on MI355X: 24 s for its 254 tests (the two child processes 6 s each); no case is left out.
"""
import pytest
import torch

from tests import _sdf_bwd_ref as R

gpu = pytest.mark.gpu
NCW_E_BADARG, NCW_E_UNSUPPORTED = -1, -2  # include/neuconw_hip.h

N = R.N_EDGE                # 13 tiles + 3 points
SLICES = (1, 33, 129, 256)  # consecutive slices of the same points (sum = N): inside a tile, one point past a tile, one past a workgroup
# W = 256 and W = 512 take every network, W = 64 the headline one and the shortest
# (W, n_layers, skip_in[, scale]): a last case with SDFNetwork.scale != 1 (xs = x scale, zsdf = d_sdf / scale)
SHAPES = [(W, nl, sk) for W in (256, 512) for nl, sk in R.NETS] + [(64, 8, (4,)), (64, 1, ()), (64, 8, (4,), 1.7)]
TRAIN_BOUND = {"f32": lambda W: 2e-4, "bf16": lambda W: 0.25, "f16": lambda W: 0.03 if W == 64 else 8e-3}  # tests/test_gpu_sdf_train.py


def _sid(s):
    W, nl, sk = s[:3]
    return "W%d-n%ds%s" % (W, nl, sk[0] if sk else "x") + ("-scale%g" % s[3] if len(s) > 3 else "")


shapes = pytest.mark.parametrize("shape", SHAPES, ids=_sid)
precs = pytest.mark.parametrize("prec_name", R.PRECS)
_GPU_NETS = {}


def _prec(name):
    import neuralrecon_w_amd as nw

    return {"f32": nw.PREC_F32, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16}[name]


def _gpu_net(shape):
    """one module per shape for the whole file: its packed plans (one per precision) are built once"""
    if shape not in _GPU_NETS:
        _GPU_NETS[shape] = R.gpu_net(R.case(*shape))
    return _GPU_NETS[shape]


def _dev(cot, lo=None, hi=None):
    return {k: v[lo:hi].contiguous().cuda() for k, v in cot.items()}


def _regions(ar, ids, names):
    """[(name, byte offset, bytes)] of the stash vectors `names` over ALL allocated tiles"""
    out = []
    for name in names:
        i = ids[name]
        for key, j in (("", i),) if isinstance(i, int) else i.items():
            off, rb = ar._off[j]
            out.append(("%s%s" % (name, key), off, ar.tiles_alloc * rb * 1024 * ar.esize))
    return out


def _step(net, W, prec_name, pts, n, cot, fill=False):
    """forward + backward of one launch -> ({field: rows of the n points}, ctx, the arena's bytes between the two kernels).
    fill: every byte of the arena is 0xFF (NaN in fp32, bf16 and fp16) before the forward."""
    from neuralrecon_w_amd.stash import StashCache

    prec = _prec(prec_name)
    if fill:
        _, _, c0 = net.fwd_stash(pts, n, prec)
        torch.cuda.synchronize()
        StashCache.release(c0["lease"])
        c0["arena"].buf.fill_(0xFF)
    sdf, grad, c = net.fwd_stash(pts, n, prec)
    ar, ids = c["arena"], c["ids"]
    assert not fill or ar is c0["arena"]
    ar.from_rows(ids["dfeat"], cot["d_feat"])
    snap = ar.buf.clone()
    net.bwd_stash(c, cot["d_sdf"], cot["d_grad"])
    L = net.n_lin
    out = {"sdf": sdf.clone(), "grad": grad.clone(), "feat": ar.to_rows(ids["feat"], W), "gamma": ar.to_rows(ids["gamma"], 64),
           "dfeat": ar.to_rows(ids["dfeat"], W), "zsdf": ar.to_rows(ids["zsdf"], 32), "one": ar.to_rows(ids["one"], 32),
           "qbar0": ar.to_rows(ids["qbar"][0], 64)}
    for name in ("h", "s", "t", "zbar"):
        for l, i in ids[name].items():
            out["%s%d" % (name, l)] = ar.to_rows(i, W)
    for l in range(1, L):
        out["qbar%d" % l] = ar.to_rows(ids["qbar"][l], W)
    torch.cuda.synchronize()
    assert {"zbar%d" % l for l in range(L - 1)} | {"t%d" % l for l in range(L - 1)} | {"h%d" % l for l in range(1, L)} <= set(out)
    return out, c, snap


def _release(c):
    from neuralrecon_w_amd.stash import StashCache

    StashCache.release(c["lease"])


# ---- a. launch decomposition -------------------------------------------------------------------------------------------------------
@gpu
@precs
@shapes
def test_launch_decomposition_invariance(shape, prec_name):
    from neuralrecon_w_amd.neuconw import points_struct

    W = shape[0]
    c = R.case(*shape, n=N)
    net, x, cot = _gpu_net(shape), c["x"].cuda(), c["cots"]["both"]
    full, ctx, _ = _step(net, W, prec_name, points_struct(x=x), N, _dev(cot))
    _release(ctx)
    for k, v in full.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    lo = 0
    for m in SLICES:
        part, ctx, _ = _step(net, W, prec_name, points_struct(x=x[lo:lo + m].contiguous()), m, _dev(cot, lo, lo + m))
        _release(ctx)
        assert set(part) == set(full)
        for k, v in full.items():
            assert torch.equal(part[k], v[lo:lo + m]), (k, shape, prec_name, lo, m)
        lo += m
    assert lo == N


@gpu
@pytest.mark.parametrize("T", ["3", "4"])
def test_w512_three_and_four_tile_kernels_in_a_subprocess(T):
    """sdf_bwd16_kernel<3> / <4> (and the forward's): the 16-bit W = 512 cases of parts a, b, c and, under `both`, d in a fresh child
    with NCW_SDF16_T set (read once per process)."""
    import os
    import subprocess
    import sys

    if os.environ.get("NCW_SDF16_T") is not None:
        pytest.skip("already inside a variant run")
    env = dict(os.environ, NCW_SDF16_T=T)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k",
                        "W512 and (bf16 or f16) and not subprocess and not first and not second"],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(here))
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- b. what the backward writes ---------------------------------------------------------------------------------------------------
@gpu
@precs
@shapes
def test_backward_writes_what_it_owns(shape, prec_name):
    from neuralrecon_w_amd.neuconw import points_struct

    W = shape[0]
    c = R.case(*shape, n=N)
    net, pts = _gpu_net(shape), points_struct(x=c["x"].cuda())
    L = net.n_lin
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[prec_name]
    for cot in R.COTS:
        out, ctx, snap = _step(net, W, prec_name, pts, N, _dev(c["cots"][cot]), fill=True)
        ar, ids = ctx["arena"], ctx["ids"]
        after = ar.buf.clone()
        _release(ctx)
        for k, v in out.items():
            assert bool(torch.isfinite(v).all()), (k, cot)
        for name, off, size in _regions(ar, ids, ("gamma", "feat", "dfeat", "h", "s", "t")):
            assert torch.equal(after[off:off + size], snap[off:off + size]), (name, cot, shape, prec_name)
        for l in range(L):
            z = float(out["qbar%d" % l].abs().max())
            assert (z == 0) == (cot == "first"), (l, cot, z)
        assert (float(out["zsdf"].abs().max()) == 0) == (cot == "second")
        assert float(out["zsdf"][:, 1:].abs().max()) == 0
        if net.scale == 1:
            assert torch.equal(out["zsdf"][:, 0], _dev(c["cots"][cot])["d_sdf"].to(dt).float())
        for l in range(L - 1):
            assert float(out["zbar%d" % l].abs().max()) > 0, (l, cot)
        # `one`: [tile][1 block][4][64 lanes][4]; feature 0 of point `lane` of a tile is element [0][lane][0], lanes 32 .. 63 hold features 4 ..
        (_, off, size), = _regions(ar, ids, ("one",))
        raw = after[off:off + size].view(dt).float().reshape(ar.tiles_alloc, 4, 64, 4)[:ar.tiles]
        want = torch.zeros_like(raw)
        want[:, 0, :32, 0] = (torch.arange(ar.tiles * 32, device="cuda") < N).float().reshape(ar.tiles, 32)
        assert torch.equal(raw, want), (cot, shape, prec_name)


# ---- c. ray-indexed points ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec_name", ["f32", "f16"])
@pytest.mark.parametrize("R_,S", R.RAY_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", [(256, 8, (4,)), (512, 8, (4,))], ids=_sid)
def test_ray_indexed_points(shape, mode, R_, S, prec_name):
    """NcwPoints mode 1 (o + d z) and mode 2 (o + d (z_i + dist_i / 2)) on rays whose points are exact in fp32
    (tests/test_sdf_bwd_ref_host.py): the cotangents stay indexed by point, so every field equals the mode-0 run bit for bit"""
    from neuralrecon_w_amd.neuconw import points_struct

    W, n = shape[0], R_ * S
    net = _gpu_net(shape)
    inp = R.dyadic_rays(R_, S)
    d = {k: v.cuda() for k, v in inp.items()}
    cot = _dev(R.cotangents(n, W)["both"])
    pts = points_struct(rays_o=d["rays_o"], rays_d=d["rays_d"], z=d["z"], sample_dist=d["sample_dist"], mode=mode)
    assert pts.per_ray == S and pts.mode == mode
    rays, ctx, _ = _step(net, W, prec_name, pts, n, cot)
    _release(ctx)
    flat, ctx, _ = _step(net, W, prec_name, points_struct(x=R.ray_points(inp, mode, torch.float32).cuda()), n, cot)
    _release(ctx)
    assert set(rays) == set(flat)
    for k, v in flat.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
        assert torch.equal(rays[k], v), (k, shape, mode, R_, S, prec_name)


@gpu
@pytest.mark.parametrize("prec_name", ["f32", "f16"])
def test_entry_points_refuse_before_any_launch(prec_name):
    """NcwPoints mode 4 (point selections are the background NeRF's): NCW_E_UNSUPPORTED; a precision that does not exist:
    NCW_E_BADARG; n = 0: 0.  All without a launch: the outputs and the whole arena keep their bytes."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd.neuconw import points_struct

    shape, n = (64, 1, ()), 65
    net, prec = _gpu_net(shape), _prec(prec_name)
    c = R.case(*shape, n=N)
    x, cot = c["x"][:n].cuda().contiguous(), _dev(c["cots"]["both"], 0, n)
    pts = points_struct(x=x)
    _, ctx, _ = _step(net, 64, prec_name, pts, n, cot)
    pn, st, lib, stream = ctx["plan"].net, ctx["stash"], L.get_lib(), L.stream_ptr(x.device)
    before = ctx["arena"].buf.clone()

    def both(prec_, pts_, n_):
        sdf, grad = torch.full((n,), 7.25, device="cuda"), torch.full((n, 3), 7.25, device="cuda")
        r_f = lib.ncw_sdf_fwd(pn, prec_, pts_, n_, L.ptr(sdf), L.ptr(grad), st, stream)
        r_b = lib.ncw_sdf_bwd(pn, prec_, pts_, n_, L.ptr(cot["d_sdf"]), L.ptr(cot["d_grad"]), st, stream)
        torch.cuda.synchronize()
        assert bool((sdf == 7.25).all()) and bool((grad == 7.25).all()) and torch.equal(ctx["arena"].buf, before)
        return r_f, r_b

    sel = L.NcwPoints.from_buffer_copy(pts)
    sel.mode = 4
    assert both(prec, sel, n) == (NCW_E_UNSUPPORTED, NCW_E_UNSUPPORTED)
    assert both(7, pts, n) == (NCW_E_BADARG, NCW_E_BADARG) and both(-1, pts, n) == (NCW_E_BADARG, NCW_E_BADARG)
    assert both(prec, pts, 0) == (0, 0)
    _release(ctx)


# ---- d. against the fp64 statement -------------------------------------------------------------------------------------------------
def _wgrads(net, ctx, prec, n):
    from neuralrecon_w_amd.stash import WgradBatch

    plan = ctx["plan"]
    plan.g_arena.zero_()
    batch = WgradBatch(net.lin0.bias.device, prec, n)
    net.add_wgrads(ctx, batch)
    batch.run()
    grads = {id(p): torch.zeros_like(p) for p in net.parameters()}
    _keep = plan.unpack_grads(grads)
    torch.cuda.synchronize()
    return {"sdf_net." + k: grads[id(p)].cpu() for k, p in net.named_parameters()}


def _closest(errs, bounds):
    k = max(errs, key=lambda k: errs[k] / bounds[k] if bounds[k] > 0 else (float("inf") if errs[k] > 0 else -1.0))
    return k


@gpu
@pytest.mark.parametrize("cot", R.COTS)
@precs
@shapes
def test_fields_and_gradients_vs_statement(shape, prec_name, cot):
    from neuralrecon_w_amd.neuconw import points_struct

    W, nl, sk = shape[:3]
    n = R.N_ORACLE
    headline = (nl, sk) == (8, (4,)) and len(shape) == 3
    c = R.case(*shape)
    r = R.ref(c, cot)
    fl, gfl = R.floors(c, cot, prec_name)
    net = _gpu_net(shape)
    out, ctx, _ = _step(net, W, prec_name, points_struct(x=c["x"].cuda()), n, _dev(c["cots"][cot]))
    got_g = _wgrads(net, ctx, _prec(prec_name), n)
    _release(ctx)
    assert set(got_g) == set(r["grads"])
    errs = R.field_errors({k: out[k].cpu() for k in r["fields"]}, r["fields"])
    gerrs = {k: R.err(got_g[k], g) for k, g in r["grads"].items()}
    train = TRAIN_BOUND[prec_name](W)
    if prec_name == "f32":
        bounds = {k: max(2e-4, 2 * fl[k]) for k in errs}
        gbounds = {k: train if headline else max(train, 2 * gfl[k]) for k in gerrs}
    else:
        bounds = {k: 2 * fl[k] for k in errs}
        gbounds = {k: train if headline and cot == "both" else max(train, 2 * gfl[k]) for k in gerrs}
    kf, kg = _closest(errs, bounds), _closest(gerrs, gbounds)
    print("SDFBWD %-17s %-4s %-6s  field %-6s gpu %.2e floor %.2e   gradient %-16s gpu %.2e floor %.2e bound %.2e"
          % (_sid(shape), prec_name, cot, kf, errs[kf], fl[kf], kg[len("sdf_net."):], gerrs[kg], gfl[kg], gbounds[kg]))
    bad = ["%s gpu %.3e floor %.3e" % (k, errs[k], fl[k]) for k in errs if not (errs[k] < bounds[k] or errs[k] == bounds[k] == 0)]
    bad += ["%s gpu %.3e floor %.3e bound %.3e" % (k, gerrs[k], gfl[k], gbounds[k]) for k in gerrs
            if not (gerrs[k] < gbounds[k] or gerrs[k] == 0)]
    assert not bad, bad


@gpu
def test_unpack_table_is_keyed_by_every_gradient_tensor():
    """part d re-uses one module with fresh gradient tensors per case and found PackPlan.unpack_grads caching its device table by the
    WEIGHT gradients' addresses alone: when the allocator hands those blocks back while the gain and bias gradients move, the cached
    table wrote d_g and d_bias through stale pointers.  Same weight tensors, new gain / bias tensors: a new table."""
    net = _gpu_net((64, 1, ()))
    plan = net.packed(_prec("f32"))
    first = {id(p): torch.zeros_like(p) for p in net.parameters()}
    second = {id(p): (first[id(p)] if n.endswith("weight_v") else torch.zeros_like(p)) for n, p in net.named_parameters()}
    t1 = plan.unpack_grads(first, launch=False)
    assert plan.unpack_grads(first, launch=False) is t1
    t2 = plan.unpack_grads(second, launch=False)
    assert t2 is not t1 and t2[0].data_ptr() != t1[0].data_ptr()
    torch.cuda.synchronize()
