/*
 * sdy_amd.h -- C ABI of the MI355X-native Spherical-DYffusion sampling path.
 *
 * The reference (Rose-STL-Lab/spherical-dyffusion) is 100 % Python and has no FFI boundary for this path;
 * the objects this library replaces are Python callables.  Each entry point below cites the reference
 * interface it stands in for (file:line under the reference root).  INTEGRATION.md shows the ctypes stub a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer; "host" pointers are ordinary host memory
 *   - all tensors are contiguous fp32; grid-space activations are NCHW = (B, C, nlat, nlon)
 *   - every function returns SDY_OK (0), a negative SDY_ERR_* for a bad argument, or a positive hipError_t
 *   - nothing here synchronises the device, allocates in a launch path, or throws; work is enqueued on the
 *     given stream (a hipStream_t passed as void*), so calls are graph-capturable
 *   - workspaces are supplied by the caller (PyTorch caching allocator on the Python side)
 *
 * Internal spectral layouts (fp32):
 *   grid-frequency  Xf[m][k][b][ri][c]   m < mtr = min(mmax, lmax), k < nlat, ri in {re, im}
 *   coefficients    Cs[l][m][b][ri][c]   l < lmax, m < mtr; entries with m > l are never read (sdy_legendre_fwd zeroes them)
 * (These are the layouts of the stage-level entry points below.  sdy_sfno_forward keeps its own spectral workspace in a
 *  private variant: the 2C axis ordered [c/16][ri][16], and (order, latitude) pairs whose Legendre table entries are below
 *  1e-12 of the order's maximum omitted altogether -- DESIGN.md section 3.)
 *
 * Dropout stream (the reference uses torch's global generator: src/models/sfno/layers.py:76-78,
 * src/models/modules/drop_path.py:19 -- not reproducible across devices, so the product defines its own):
 *   Philox4x32-7 (the Random123 generator with seven rounds, the smallest count that passes BigCrush; round constants as in
 *   Random123), key = (seed_lo, seed_hi), counter = (c0, c1, stream, call)
 *     element dropout : n = pixel (h*nlon + w); c0 = n with bit 5 cleared, c1 = b_global*(C/4) + (ch>>2), word = ch & 3,
 *                       half-word = bit 5 of n (0: low 16 bits, 1: high 16 bits),
 *                       stream = 2*layer + kind (kind 0 = MLP hidden, 1 = MLP output);
 *                       keep <=> half-word >= floor(p * 2^16)   (one call serves 4 channels x the pixel pair n, n + 32)
 *     drop path       : c0 = b_global, c1 = 0xFFFFFFFF, stream = 0x1000 + layer, word 0;
 *                       keep <=> word >= floor(p * 2^32)
 *   kept values are scaled by 1/(1-p).
 *
 * Forward-conditioning noise stream (the eps of DYffusion's "data+noise-v1/v2", src/diffusion/dyffusion.py:321-330, where the
 * reference draws torch.randn_like): same generator and key, one call per 4 consecutive pixels of one (trajectory, channel):
 *     counter = (q, b_global*C + c, 0x2000, call)   q = pixel / 4 (pixel = h*nlon + w), C = channels of the group,
 *                                                   c < C its channel, call = the network's call number of the row
 *     u(word) = ((word >> 8) + 1) * 2^-24 in (0, 1];  Box-Muller on the call's words (w0, w1) and (w2, w3):
 *     eps[4q + 0], eps[4q + 1] = r0 cos(2 pi u(w1)), r0 sin(2 pi u(w1))    r0 = sqrt(-2 ln u(w0))
 *     eps[4q + 2], eps[4q + 3] = r1 cos(2 pi u(w3)), r1 sin(2 pi u(w3))    r1 = sqrt(-2 ln u(w2))
 *   stream word 0x2000 is outside every stream word of the dropout stream (< 64 and 0x1000 + layer, layer < 32).
 */
#ifndef SDY_AMD_H
#define SDY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported. */
#pragma GCC visibility push(default)

#define SDY_OK 0
#define SDY_ERR_ARG (-1)         /* null pointer / non-positive extent */
#define SDY_ERR_UNSUPPORTED (-2) /* size the kernels do not cover (e.g. nlon with a prime factor > 5) */
#define SDY_ERR_ALIGN (-3)       /* extent along a contiguous dimension not a multiple of 4, or a pointer that a kernel reads
                                    or writes as float4 not 16-byte aligned (stated at the prototypes concerned) */
#define SDY_ERR_WORKSPACE (-4)   /* workspace too small */
#define SDY_ERR_NAME (-5)        /* unknown parameter name */
#define SDY_ERR_SHAPE (-6)       /* parameter has the wrong number of elements */
#define SDY_ERR_STATE (-7)       /* object not fully initialised (missing parameters) */

#define SDY_GRID_EQUIANGULAR 0
#define SDY_GRID_LEGENDRE_GAUSS 1

int sdy_version(void);
const char* sdy_error_string(int code);
/* The argument structures below carry no size field: a caller built against another revision of this header would hand the
 * launchers uninitialised tail bytes (fields are only ever appended).  Contract: zero-initialise every structure with the
 * sizeof of THIS header, and call sdy_abi_check once after loading the library with your own sizeofs of every argument
 * structure below, in header order:
 *   {sdy_conv_args, sdy_mlp_args, sdy_pair_args, sdy_sfno_config, sdy_sfno_fwd_args, sdy_var_table, sdy_step_finish_args,
 *    sdy_derived_args, sdy_corrector_args, sdy_dry_air_args, sdy_hist_args, sdy_coarsen_args, sdy_video_args, sdy_zonal_args,
 *    sdy_member_sum_args, sdy_member_stats_args, sdy_spectrum_args, sdy_variability_args, sdy_variability_maps_args,
 *    sdy_variability_stats_args, sdy_region_series_args, sdy_event_args, sdy_fss_args, sdy_member_gram_args,
 *    sdy_rank_hist_args}
 * SDY_OK when n == SDY_ABI_STRUCTS and every size equals the library's, SDY_ERR_ARG otherwise (the Python bindings do this at
 * import).  sdy_abi_sizes writes the library's own list, for the message of a failed check (SDY_ERR_ARG: n != SDY_ABI_STRUCTS). */
#define SDY_ABI_STRUCTS 25
int sdy_abi_check(const size_t* sizes, int n);
int sdy_abi_sizes(size_t* sizes, int n);

/* ---------------------------------------------------------------------------------------------------------
 * Spherical-harmonic transform plan.
 * Replaces torch_harmonics.RealSHT / InverseRealSHT construction (third-party, un-vendored; reference call
 * sites src/models/sfno/sfnonet.py:551-554; attributes read at src/models/sfno/s2convolutions.py:73-83).
 * One plan holds the forward (quadrature-weighted) and inverse Legendre tables of one grid, in fp32 on the
 * device (computed in fp64 on the host, cast like `.float()` at sfnonet.py:551-554), plus FFT twiddles. */
typedef struct sdy_sht_plan sdy_sht_plan;

/* Host-only: fp64 tables exactly as torch_harmonics builds them.  pct: [mmax][lmax][nlat], w: [nlat]
 * quadrature weights, theta: [nlat] colatitudes (any may be NULL).  No GPU needed. */
int sdy_sht_tables_host(int nlat, int nlon, int lmax, int mmax, int grid, double* pct, double* w, double* theta);

int sdy_sht_plan_create(int nlat, int nlon, int lmax, int mmax, int grid, sdy_sht_plan** out);
/* gemm_mode: 0 = Legendre GEMMs on fp32 MFMA; 1 = split-fp16 3-pass MFMA (fp32-class accuracy, see sdy_sfno_config).
 * sdy_sht_plan_create uses $SDY_GEMM_MODE ("f32" -> 0, otherwise 1). */
int sdy_sht_plan_create_ex(int nlat, int nlon, int lmax, int mmax, int grid, int gemm_mode, sdy_sht_plan** out);
void sdy_sht_plan_destroy(sdy_sht_plan* plan);
/* dims[0..5] = nlat, nlon, lmax, mmax, mtr, grid */
int sdy_sht_plan_dims(const sdy_sht_plan* plan, int dims[6]);
/* Which kernels the plan resolved to (read-only): out[0] = Legendre back end of both directions -- 0 folded fragment stream
 * (leg_par.hip), 1 fragment stream (leg_h3.hip), 2 split-fp16 batched GEMM (gemm_h3.hip), 3 fp32 batched GEMM (gemm.hip);
 * out[1] = 1 when the longitude FFTs of C % 16 == 0 fields run in the 360-point kernels of fft360.hip, else 0. */
int sdy_sht_plan_kernels(const sdy_sht_plan* plan, int out[2]);
/* floats needed by sdy_sht_forward / sdy_sht_inverse for B*C fields */
size_t sdy_sht_workspace_floats(const sdy_sht_plan* plan, int B, int C);

/* RealSHT.forward (torch_harmonics; called at src/models/sfno/s2convolutions.py:165):
 * x dev (B,C,nlat,nlon) f32 -> out dev (B,C,lmax,mmax) complex64 (re,im interleaved). C % 4 == 0. */
int sdy_sht_forward(const sdy_sht_plan* plan, const float* x, float* out_c64, int B, int C, float* ws,
                    size_t ws_floats, void* stream);
/* InverseRealSHT.forward (called at src/models/sfno/s2convolutions.py:168,186):
 * in dev (B,C,lmax,mmax) complex64 -> y dev (B,C,nlat,nlon) f32. */
int sdy_sht_inverse(const sdy_sht_plan* plan, const float* in_c64, float* y, int B, int C, float* ws,
                    size_t ws_floats, void* stream);

/* Stage-level entry points on the internal layouts (what the fused network path launches). */
/* longitude real FFT x (2*pi/nlon) fused with the per-(b,c) affine a*x+d of InstanceNorm + time scale/shift
 * (src/models/sfno/sfnonet.py:292,298-299).  a, d: dev [B*C], both or neither (else SDY_ERR_ARG).  xn_out: dev
 * (B,C,nlat,nlon) or NULL.  Xf: dev [mtr][nlat][B][2][C].  The kernels move four channels at a time as 16-byte words:
 * C % 4 == 0 and x, xn_out, Xf 16-byte aligned, else SDY_ERR_ALIGN before anything is launched. */
int sdy_rfft_lon(const sdy_sht_plan* plan, const float* x, const float* a, const float* d, float* xn_out,
                 float* Xf, int B, int C, void* stream);
/* Legendre analysis: Cs[l][m][n] = sum_k Wq[m][l][k] Xf[m][k][n]  (einsum '...km,mlk->...lm'); exact zeros where m > l */
int sdy_legendre_fwd(const sdy_sht_plan* plan, const float* Xf, float* Cs, int B, int C, void* stream);
/* Legendre synthesis: Yf[m][k][n] = sum_l P[m][l][k] Cs[l][m][n]  (einsum '...lm,mlk->...km') */
int sdy_legendre_inv(const sdy_sht_plan* plan, const float* Cs, float* Yf, int B, int C, void* stream);
/* inverse longitude FFT (irfft n=nlon, norm="forward") + optional per-channel bias (s2convolutions.py:188-189).
 * C % 4 == 0 and Yf, y 16-byte aligned, else SDY_ERR_ALIGN before anything is launched (see sdy_rfft_lon). */
int sdy_irfft_lon(const sdy_sht_plan* plan, const float* Yf, const float* bias, float* y, int B, int C,
                  void* stream);
/* The InstanceNorm statistics chain of the fused forward, kernel by kernel (what sdy_sfno_forward launches between its GEMMs;
 * statistics are dev double [B][C][2] = (sum, sum of squares) over HW of a stored plane, see sdy_conv_args.stats).  None of
 * these kernels has a scalar tail, so every call is refused before anything is launched when it would need one: HW % 4 != 0, a
 * batch stride that is not a multiple of 4, or a tensor, statistics or partials pointer off a 16-byte boundary (planes move as
 * float4, a statistics slot is one pair of doubles) is SDY_ERR_ALIGN; a NULL required pointer, a non-positive extent, n_rows >
 * 128 or a tile-major stride below ceil(HW / 64) * C * 64 is SDY_ERR_ARG.
 *
 * sdy_irfft_lon_act: sdy_irfft_lon with the block's activation on its stores: GELU(ring + bias[c]) (exact erf) goes TILE-MAJOR
 * to zt ([b][64-pixel tile][C][64], zt_bstride >= ceil(HW / 64) * C * 64 floats per image, the layout sdy_mlp_args.x_tiled reads;
 * the last tile's pixels past HW are not written) and ring k's (sum, sum of squares) of what was stored to part[b][k][c][2]
 * (dev double, B * nlat * C * 2, every slot WRITTEN exactly once, not added).  Yf in the channel order of this header,
 * [m][k][b][ri][c], as for sdy_irfft_lon.  Only the 360-point kernels have this form: SDY_ERR_UNSUPPORTED unless
 * sdy_sht_plan_kernels reports out[1] == 1 and C % 16 == 0.  zt and part are both required. */
int sdy_irfft_lon_act(const sdy_sht_plan* plan, const float* Yf, const float* bias, float* zt, long zt_bstride, double* part,
                      int B, int C, void* stream);
/* part[b][k][c][2], k < K, summed in the order of k (bit-reproducible) -> a = gamma*rstd, d = beta - mean*a (no time scale /
 * shift: this is the block's second norm).  `part` is left as it is. */
int sdy_instnorm_from_partials(const double* part, int K, int B, int C, int HW, const float* gamma, const float* beta,
                               float eps, float* a, float* d, void* stream);
/* out = GELU(y) (exact erf) for B images of C channels, y (B, C, HW) with y_bstride floats per image; out NCHW (out_bstride per
 * image) or, with out_tiled, tile-major as above.  stats (or NULL): the (sum, sum of squares) of what is stored are ADDED to
 * stats[b][c].  out may be y itself when it is not tiled. */
int sdy_gelu_stats(const float* y, long y_bstride, float* out, long out_bstride, int out_tiled, double* stats, int B, int C,
                   int HW, void* stream);
/* The drop-path skip: out[b] = a[b][c] * x[s] + d[b][c] (one fma; a, d dev [rows of out][C], both NULL = a plain copy) for the
 * n_rows <= 128 batch rows b = rows[i] (host array); source row s = b, or src_row0 + i when src_row0 >= 0 (x in the launch's own
 * order).  The (sum, sum of squares) of every stored plane are ADDED to stats[b][c] unless stats is NULL; rows that are not
 * listed are not touched. */
int sdy_affine_copy_stats(const float* x, long x_bstride, const float* a, const float* d, float* out, long out_bstride,
                          double* stats, int C, int HW, const unsigned char* rows, int n_rows, int src_row0, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * _contract_dhconv (src/models/sfno/contractions.py:159-169 via factorizations.py:165-186; called at
 * src/models/sfno/s2convolutions.py:173-178):  out[b,o,l,m] = sum_i x[b,i,l,m] * w[i,o,l]  (complex).
 * sdy_dhconv_pack_weight: host (Ci,Co,L,2) reference layout -> dev packed [l][2][Ci][Co].
 * sdy_dhconv: Cs_in / Cs_out in the coefficient layout above (channel counts Ci / Co, both % 4 == 0). */
int sdy_dhconv_pack_weight(const float* w_host, int Ci, int Co, int L, float* w_packed_dev, void* stream);
int sdy_dhconv(const float* Cs_in, const float* w_packed, float* Cs_out, int L, int mtr, int B, int Ci, int Co,
               void* stream);
/* Same contraction on the f16 matrix cores in split precision (3 passes, fp32-class accuracy): the weight is expanded to
 * its real 2Ci x 2Co form, transposed and split into fp16 hi | lo on the host. */
size_t sdy_dhconv_h3_pack_bytes(int Ci, int Co, int L);
int sdy_dhconv_h3_pack_weight(const float* w_host, int Ci, int Co, int L, void* packed_dev, float* scale);
int sdy_dhconv_h3(const float* Cs_in, const void* packed, float scale, float* Cs_out, int L, int mtr, int B, int Ci,
                  int Co, void* stream);

/* Same contraction for Ci = Co = 256 as a persistent fragment-stream kernel (dh_h3.hip): a workgroup owns 64 rows and
 * all 512 output columns, so every coefficient row is read once; the packed weight (1 MB per degree, MFMA fragment
 * order) streams L2 -> registers and each degree is served by one XCD.  Same reference lines as sdy_dhconv
 * (src/models/sfno/contractions.py:159-169).  `scale` is what the pack returned. */
int sdy_dhconv_frag_supported(int Ci, int Co);
size_t sdy_dhconv_frag_pack_bytes(int L);
int sdy_dhconv_frag_pack(const float* w_host, int L, void* packed_dev, float* scale);
int sdy_dhconv_frag(const float* Cs_in, const void* packed, float scale, float* Cs_out, int L, int mtr, int B,
                    void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * nn.InstanceNorm2d(C, eps, affine=True, track_running_stats=False) statistics folded with the block's time
 * scale/shift (src/models/sfno/sfnonet.py:280-299,641-648) into per-(b,c) coefficients:
 *   xn = a*x + d,  a = gamma*rstd*(1+scale),  d = (beta - mean*gamma*rstd)*(1+scale) + shift
 * scale_shift: dev, element (b, j) at scale_shift[b*ss_stride + j], j < 2C (scale | shift), or NULL. */
int sdy_instnorm_coeffs(const float* x, int B, int C, int HW, const float* gamma, const float* beta,
                        const float* scale_shift, long ss_stride, float eps, float* a, float* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * 1x1 convolution = per-pixel GEMM with fused prologue/epilogue.  Replaces nn.Conv2d(k=1) + bias + GELU +
 * Dropout + DropPath + residual adds of src/models/sfno/sfnonet.py:303-335,609-618,734-744 and
 * src/models/sfno/layers.py:73-80.
 *   out[b,o,p] = post( act( sum_i wt[i,o] * (pa[b,i]*x[b,i,p] + pd[b,i]) + bias[o] + add_pre[b,o,p] ) )
 *   post(v)    = batch_scale[b] * dropout(v) + add_post[b,o,p]
 * wt is the TRANSPOSED weight, dev [Cin][ldw] (ldw >= Cout, ldw % 4 == 0, columns >= Cout zero). */
typedef struct sdy_conv_args {
  const float* x;  long x_bstride;   /* dev (B, >=Cin, HW) ; batch stride in floats */
  const float* wt; int ldw;          /* dev [Cin][ldw] */
  float* out;      long out_bstride; /* dev (B, >=Cout, HW) */
  int B, Cin, Cout, HW;
  const float* pa; const float* pd;  /* dev [B*Cin] each or NULL (prologue affine) */
  const float* bias;                 /* dev [Cout] or NULL */
  const float* add; long add_bstride;/* dev (B or 1, Cout, HW) or NULL; add_bstride 0 broadcasts over b */
  int add_mode;                      /* 0 none, 1 before activation, 2 after dropout/batch_scale */
  int act;                           /* 0 none, 1 exact-erf GELU */
  float drop_p;                      /* 0 = no dropout */
  const float* keep_mask;            /* dev (B,Cout,HW) 0/1 injected mask (tests) or NULL = Philox stream */
  uint64_t seed; uint32_t call; uint32_t stream_id; uint32_t batch_offset;
  int rows_per_call;                   /* 0: every batch row belongs to `call`.  n > 0: the batch stacks several calls of n
                                          rows each: row b draws the stream of (call + b / n, trajectory batch_offset + b % n)
                                          -- bit-identical to issuing those calls one after the other (the two interpolator
                                          calls of a DYffusion sampling step share their inputs: dyffusion.py:497,515) */
  const float* batch_scale;          /* dev [B] or NULL (drop-path scale) */
  int kernel_tag;                    /* 0 generic; 1 = MLP fc1, 2 = MLP fc2, 3 = inner skip: identical code under a
                                        distinct symbol name so profilers attribute time per use */
  const void* w_h3;                  /* dev, optional: weight packed by sdy_h3_pack_weight -> the GEMM runs on the f16
                                        matrix cores in split precision (3 passes, fp32-class accuracy); wt may be NULL */
  float w_h3_scale;                  /* scale returned by sdy_h3_pack_weight */
  const void* w_frag;                /* dev, optional, Cout == 256, Cin <= 384 (a pre-affine pa/pd needs Cin == 256): weight packed by sdy_conv256_h3_pack[_cin] -> the
                                        persistent fragment-stream kernel (no dropout / batch_scale / keep_mask) */
  float w_frag_scale;
  double* stats;                     /* dev [B*Cout*2] or NULL, w_frag path only: (sum, sum of squares) over HW of every
                                        output plane are ADDED here (zero it first; sdy_instnorm_from_stats turns them into
                                        the next InstanceNorm's coefficients) */
  int out_tiled;                     /* w_frag path only: write `out` TILE-MAJOR, [b][tile of 64 pixels][Cout][64] (an image's last
                                        tile padded to 64; out_bstride >= ceil(HW / 64) * Cout * 64), the layout sdy_mlp_args.x_tiled
                                        reads: a tile of the intermediate tensor between the two persistent kernels is then one
                                        contiguous 64 KB block for its producer and its consumer.  `out` must not alias `add`. */
  const unsigned char* x_rows;       /* host [B] or NULL, w_frag path only, B <= 128: image z of this launch reads batch row x_rows[z] of
                                        x / pa / pd (add, out and stats stay indexed by z).  sdy_sfno_forward runs a block whose
                                        DropPath draw (src/models/modules/drop_path.py:15-22) zeroes some trajectories' branch on
                                        the active trajectories only: its per-block tensors are compact, the block input is not. */
} sdy_conv_args;
int sdy_conv1x1(const sdy_conv_args* args, void* stream);

/* Split-precision weight packing for sdy_conv1x1 (w_h3): host (Cout, Cin) row-major fp32 -> dev fp16 hi|lo planes,
 * [Mpad][Kpad] each (Mpad = 128 for Cout <= 128, else Cout rounded up to 256; Kpad = Cin rounded up to 64), multiplied by a power of two
 * (*scale) chosen so that max|w|*scale is in [2^12, 2^13). */
/* 256 -> 256 weight (Cout, Cin) row-major -> per-wave MFMA fragment stream for sdy_conv_args.w_frag */
int sdy_conv256_h3_supported(int Cin, int Cout);
size_t sdy_conv256_h3_pack_bytes(void);                                                    /* for Cin <= 256 */
size_t sdy_conv256_h3_pack_bytes_cin(int Cin);                                             /* for any supported Cin */
int sdy_conv256_h3_pack(const float* w_host, void* packed_dev, float* scale);             /* (256, 256) weight */
int sdy_conv256_h3_pack_cin(const float* w_host, int Cin, void* packed_dev, float* scale); /* (256, Cin), Cin <= 384 */
size_t sdy_h3_pack_bytes(int Cout, int Cin);
int sdy_h3_pack_weight(const float* w_host, int Cout, int Cin, void* packed_dev, float* scale);

/* Fused MLP of one SFNO block (src/models/sfno/layers.py:73-80 as called from src/models/sfno/sfnonet.py:313-335):
 *   out[b] = batch_scale[b] * dropout2( W2 . dropout1( GELU( W1 . (pa[b]*x[b] + pd[b]) + b1 ) ) + b2 )
 *            + (add_a[b]*add[b] + add_d[b])
 * in ONE launch; the hidden activation stays on the compute unit (never written to HBM).  Split-fp16 arithmetic and
 * Philox stream identical to two sdy_conv1x1 calls with (stream_fc1, stream_fc2).  Supported shape: E = 256,
 * hidden = 512 (sdy_mlp_h3_supported); anything else returns SDY_ERR_UNSUPPORTED and the caller uses sdy_conv1x1. */
typedef struct sdy_mlp_args {
  const float* x;  long x_bstride;     /* dev (B, E, HW) */
  const float* pa; const float* pd;    /* dev [B*E] each or NULL (norm affine folded into the load) */
  const void* w; float w1_scale; float w2_scale;     /* sdy_mlp_h3_pack output and the two scales it returned */
  const float* b1; const float* b2;                  /* dev [hidden], dev [E] */
  float* out;      long out_bstride;   /* dev (B, E, HW) */
  const float* add; long add_bstride;  /* dev (B, E, HW) residual or NULL */
  const float* add_a; const float* add_d; /* dev [B*E] each or NULL: the residual is add_a*add + add_d (a norm folded
                                           into its consumer instead of being materialised) */
  int B, E, hidden, HW;
  float drop_p;                        /* 0 = no dropout */
  uint64_t seed; uint32_t call; uint32_t stream_fc1; uint32_t stream_fc2; uint32_t batch_offset;
  int rows_per_call;                   /* as in sdy_conv_args */
  const float* batch_scale;            /* dev [B] or NULL (drop-path scale) */
  double* stats;                       /* dev [B*E*2] or NULL: (sum, sum of squares) over HW of every output plane are
                                          ADDED here (InstanceNorm statistics of the next block, sfnonet.py:292): zero
                                          it before the launch, turn it into coefficients with sdy_instnorm_from_stats */
  int x_tiled;                         /* x is TILE-MAJOR (sdy_conv_args.out_tiled; x_bstride = floats per image); needs `add` */
  const float* keep_hidden;            /* tests only, dev (B, hidden, HW) and (B, E, HW) 0/1 masks or NULL: with drop_p > 0 the */
  const float* keep_out;               /* keep decisions come from these (e.g. masks the reference's nn.Dropout drew) instead of
                                          the Philox stream -- same kernel code, a separate (untimed) instantiation */
  const unsigned char* out_rows;       /* host [B] or NULL, B <= 128: image z of this launch (x, pa, pd indexed by z) IS batch row
                                          out_rows[z] -- add, add_a, add_d, out, stats, batch_scale, keep_* and the dropout stream
                                          (call, trajectory) are taken at that row (see sdy_conv_args.x_rows) */
  int add_by_launch_row;               /* with out_rows and without add_a / add_d: `add` is indexed by the launch's image z, like x
                                          (a residual that was materialised in the launch's own row order) */
} sdy_mlp_args;
/* (sum, sumsq) statistics -> the same per-(b,c) affine coefficients as sdy_instnorm_coeffs; clears `stats` for reuse. */
int sdy_instnorm_from_stats(double* stats, int B, int C, int HW, const float* gamma, const float* beta,
                            const float* scale_shift, long ss_bstride, float eps, float* a_out, float* d_out, void* stream);
int sdy_mlp_h3_supported(int E, int hidden);
size_t sdy_mlp_h3_pack_bytes(int E, int hidden);
/* w1_host: (hidden, E) row-major = mlp.fwd.0.weight;  w2_host: (E, hidden) row-major = mlp.fwd.{2|3}.weight.
 * Both are split to fp16 hi|lo (times a power of two each, returned) and interleaved into one per-wave stream in the
 * order the kernel consumes them. */
int sdy_mlp_h3_pack(const float* w1_host, const float* w2_host, int E, int hidden, void* packed_dev, float* scale1,
                    float* scale2);
int sdy_mlp_h3(const sdy_mlp_args* args, void* stream);

/* Two 1x1 convolutions with a GELU between them in ONE launch -- the encoder (src/models/sfno/sfnonet.py:609-618, with the
 * position embedding of :824 as the addend) and the decoder (:734-744 on [block output | inputs], :831-837):
 *   out[b] = W2 . GELU( W1 . x[b] + b1 ) + add[b or broadcast]
 * The 256-channel hidden activation stays on the compute unit.  Split-fp16 arithmetic of sdy_conv1x1 (w_h3), except that the
 * activations are not staged with the fixed pre-scale: x by a power of two per 64-pixel tile (and channel part) from the tile's
 * own maximum, the hidden activation by one from the bound max_row ||W1 row||_1 * max|x| + max|b1| (the L1 norm is computed by
 * sdy_pair_h3_pack and travels in the last 64 bytes of the packed buffer).  Inputs of any finite magnitude keep 22 bits
 * relative to their tile's maximum; SDY_FLAG_F16_RANGE is never raised here, SDY_FLAG_NONFINITE is for inf / NaN inputs.  Supported
 * shapes (sdy_pair_h3_supported): hidden == 256 and either Cout == 256 with Cin <= 144, or Cout <= 64 with Cin <= 416;
 * anything else returns SDY_ERR_UNSUPPORTED and the caller issues two sdy_conv1x1 calls. */
typedef struct sdy_pair_args {
  const float* x;  long x_bstride;     /* dev (B, >=Cin, HW) */
  const void* w; float w1_scale; float w2_scale;     /* sdy_pair_h3_pack output and the two scales it returned */
  const float* b1;                     /* dev [hidden] or NULL */
  float* out;      long out_bstride;   /* dev (B, >=Cout, HW) */
  const float* add; long add_bstride;  /* dev (B or 1, Cout, HW) or NULL; add_bstride 0 broadcasts over b */
  int B, Cin, hidden, Cout, HW;
  double* stats;                       /* dev [B*Cout*2] or NULL (Cout == 256 only): (sum, sum of squares) over HW of every
                                          output plane are ADDED here, as in sdy_mlp_args */
} sdy_pair_args;
int sdy_pair_h3_supported(int Cin, int hidden, int Cout);
size_t sdy_pair_h3_pack_bytes(int Cin, int hidden, int Cout);
/* w1_host: (hidden, Cin) row-major;  w2_host: (Cout, hidden) row-major */
int sdy_pair_h3_pack(const float* w1_host, const float* w2_host, int Cin, int hidden, int Cout, void* packed_dev,
                     float* scale1, float* scale2);
int sdy_pair_h3(const sdy_pair_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Whole network.  Replaces SphericalFourierNeuralOperatorNet.__init__/forward
 * (src/models/sfno/sfnonet.py:426-841) + BaseModel.concat_condition_if_needed (src/models/_base_model.py:166-192)
 * for the configuration the shipped YAML selects (filter_type=linear, operator_type=dhconv, factorization=None,
 * instance_norm, use_mlp, pos_embed, big_skip, scale_factor=1, encoder_layers=1). */
typedef struct sdy_sfno_config {
  int nlat, nlon;
  int in_chans;        /* inputs + conditional channels, as the encoder sees them */
  int out_chans;
  int embed_dim;
  int num_layers;
  int mlp_hidden;      /* int(embed_dim * mlp_ratio) */
  int lmax, mmax;      /* modes_lat, modes_lon (sfnonet.py:526-527) */
  int data_grid;       /* SDY_GRID_* of the first forward / last inverse transform */
  int with_time_emb;
  int time_dim;        /* embed_dim * time_dim_mult */
  float dropout_mlp;   /* MLP dropout rate (active only when a forward call enables dropout) */
  float drop_path_rate;
  int big_skip, pos_embed;
  int gemm_mode;       /* 0: fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere; 1: the 1x1 convolutions run as split-fp16
                          3-pass MFMA GEMMs (fp32-class accuracy at the f16 matrix rate) */
} sdy_sfno_config;

typedef struct sdy_sfno sdy_sfno;
int sdy_sfno_create(const sdy_sfno_config* cfg, sdy_sfno** out);
void sdy_sfno_destroy(sdy_sfno* net);
/* Load one tensor by its reference state_dict name, host fp32, `numel` elements.
 * The library re-lays it out for the kernels.  Names of non-persistent SHT buffers are accepted and ignored. */
int sdy_sfno_set_param(sdy_sfno* net, const char* name, const float* host, size_t numel);
/* 0 when every required parameter has been set; otherwise SDY_ERR_STATE (missing name via sdy_sfno_missing). */
int sdy_sfno_ready(const sdy_sfno* net);
const char* sdy_sfno_missing(const sdy_sfno* net);
size_t sdy_sfno_workspace_floats(const sdy_sfno* net, int B);
/* Largest B one sdy_sfno_forward call takes: 128 on the default kernel path (the drop-path row maps; the 32-bit offsets inside
 * the spectral workspace would allow 258 rows at 180 x 360, embed 256), 60 there with row-major coefficient tensors; larger
 * batches run as consecutive calls on row ranges, each with its own batch_offset (the Python module does). */
int sdy_sfno_max_batch(const sdy_sfno* net);

typedef struct sdy_sfno_fwd_args {
  /* up to three channel groups concatenated on dim 1 (inputs | condition | static_condition) */
  const float* in[3]; int in_chans[3];   /* dev (B, in_chans[i], nlat, nlon); unused slots NULL / 0 */
  const float* time;                     /* dev [B] or NULL when !with_time_emb */
  float* out;                            /* dev (B, out_chans, nlat, nlon) */
  int B;
  int enable_dropout;                    /* inference_dropout_scope (src/models/_base_model.py:273-286) */
  uint64_t seed; uint32_t call; uint32_t batch_offset;
  int rows_per_call;       /* 0, or n: the B rows are B / n stacked calls (call, call + 1, ...) of n trajectories each, see
                              sdy_conv_args; B must be a multiple of n */
  const float* const* keep_masks;        /* optional injected masks (tests): [num_layers*2] dev pointers
                                            (hidden, out) per layer, or NULL */
  const float* drop_path_keep;           /* optional injected drop-path keep flags, dev [num_layers][B], or NULL */
  float* ws; size_t ws_floats;
  int reuse_encoder;       /* 1: every `in` tensor holds the same values as in the PREVIOUS forward of this network on this
                              workspace with the same B (the two interpolations of a cold-sampling step share their inputs,
                              src/diffusion/dyffusion.py:497,515): the input concat and the encoder are skipped and the forward
                              restarts from the stored encoder output -- bit-identical results (time, dropout call number and
                              masks may differ: they enter after the encoder).  SDY_ERR_STATE if there is no such forward. */
  int shared_inputs;       /* 1 (needs rows_per_call = n < B): the stacked calls share their inputs -- every `in` tensor holds n
                              rows, and row b of the forward reads input row b % n (the two interpolations of a cold-sampling
                              step as ONE forward of 2n rows: same (x_0, forecast) and static condition, other time and dropout
                              call).  The encoder then runs on n rows (when block 0 changes grids, on the default path;
                              otherwise on all B rows); results are bit-identical to stacking copies. */
  /* One GENERATED channel group (DYffusion forward conditioning, src/diffusion/dyffusion.py:310-353): it holds
   *   a_b * gen_src[b, c, p] + s_b * eps(seed, call(b), batch_offset + b % n, c, p)     (n = rows_per_call or B,
   *   call(b) = call + b / n; eps: the forward-conditioning noise stream above), both products rounded before the sum.
   * The group sits in front of the gen_pos-th PRESENT `in` group (0 = first, number of present groups = last); the channel
   * total including gen_chans must be in_chans.  s_b == 0 copies a_b * x and draws nothing ("data" with a_b = 1).
   * Zeroed fields (gen_src NULL): no generated group, the concat of earlier revisions.  Its values change with every call, so
   * reuse_encoder / shared_inputs with a generated group are SDY_ERR_ARG. */
  const float* gen_src;    /* dev (B, gen_chans, nlat, nlon) or NULL */
  int gen_chans;
  int gen_pos;
  const float* gen_coef;   /* dev [B][2]: (a_b, s_b) */
  const float* gen_noise;  /* optional injected eps (tests), dev (B, gen_chans, nlat, nlon), or NULL: the Philox draw */
} sdy_sfno_fwd_args;
int sdy_sfno_forward(sdy_sfno* net, const sdy_sfno_fwd_args* args, void* stream);

/* Debug/parity taps: time embedding + per-block (scale|shift) as the network computes them.
 * t_repr dev [B*time_dim] (or NULL), ss dev [B*num_layers*2*embed_dim] (or NULL). */
int sdy_sfno_time_embed(sdy_sfno* net, const float* time, int B, float* t_repr, float* ss, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Sampler arithmetic of BaseDYffusion.sample_loop (src/diffusion/dyffusion.py:517-519, :655-661). */
/* out = x_s + (x_ip_next - x_ip_s); any of the three may alias out.  x_ip_s NULL means "x_ip_s == x_s" (s = 0).
 * 16-byte aligned pointers are read and written as float4; if any of the four is not aligned, the whole range goes through
 * 4-byte accesses instead (same values, bit for bit). */
int sdy_cold_update(const float* x_s, const float* x_ip_next, const float* x_ip_s, float* out, size_t n,
                    void* stream);
/* channel concat of up to 4 NCHW tensors (torch.cat(dim=1)).  HW % 4 == 0 and every src[i] and out 16-byte aligned (float4
 * copies), else SDY_ERR_ALIGN before anything is launched; the same holds for the inputs of sdy_sfno_forward, which are
 * concatenated by the same kernels. */
int sdy_concat_channels(const float* const* src, const int* chans, int nsrc, float* out, int B, int HW,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stepper glue either side of the sampler ("next" row of the scope table): the device arithmetic of
 * run_on_batch_multistep (src/ace_inference/core/stepper_multistep.py:298-466): StandardNormalizer
 * (src/ace_inference/core/normalizer.py:96-110), Packer (src/utilities/packer.py:70-77), Prescriber
 * (src/ace_inference/core/prescriber.py:68-92), relative LpLoss (src/ace_inference/training/utils/darcy_loss.py:214-228).
 * Variables are separate dev tensors (B, T1, nlat*nlon) as in the reference's data dict.
 * Alignment: these kernels move float4.  HW % 4 == 0, and EVERY device pointer of float data handed to sdy_norm_pack,
 * sdy_init_timeline, sdy_step_finish and sdy_lp_rel_terms -- the per-variable data[] of a table, out, the per-entry timelines,
 * gen, prev_in, next_in, ar_init, presc_target, presc_mask -- must be 16-byte aligned; otherwise SDY_ERR_ALIGN is returned
 * before anything is launched and nothing is written.  (A freshly allocated tensor is aligned; a contiguous VIEW that starts
 * at an odd element of a larger buffer is not: copy it first.) */
#define SDY_MAX_VARS 96
typedef struct sdy_var_table {
  int nvars;
  const float* data[SDY_MAX_VARS];  /* dev (B, T1, HW), denormalised */
  float mean[SDY_MAX_VARS];         /* 0 / 1 for variables without statistics (passed through) */
  float std[SDY_MAX_VARS];
} sdy_var_table;
/* normalise + pack: out[b][v][p] = (data_v[b][t][p] - mean_v) / std_v,  out dev (B, nvars, HW) */
int sdy_norm_pack(const sdy_var_table* vars, int t, int T1, int B, int HW, float* out, void* stream);

typedef struct sdy_step_finish_args {
  int B, HW, T1, t;                   /* t = time index being written (1..n_forward_steps) */
  const float* gen; int n_out;        /* dev (B, n_out, HW): the module's normalised prediction for step t */
  const float* prev_in; float* next_in; int n_in;  /* dev (B, n_in, HW) packed model state (in_packer order) */
  int n_entries;                      /* one entry per distinct variable in (in_packer names) U (out names) */
  int out_idx[SDY_MAX_VARS];          /* index in the out packer or -1 (input-only: carried over, e.g. HGTsfc) */
  int in_idx[SDY_MAX_VARS];           /* index in the in packer or -1 (diagnostic-only output) */
  float* gen_norm_tl[SDY_MAX_VARS];   /* per entry with out_idx >= 0: dev (B, T1, HW) normalised timeline */
  float* gen_tl[SDY_MAX_VARS];        /* ... and denormalised timeline (value*std + mean) */
  float mean[SDY_MAX_VARS], std[SDY_MAX_VARS];
  int presc_entry;                    /* entry overwritten by the prescriber, or -1 */
  const float* presc_target;          /* dev (B, T1, HW) denormalised data of the prescribed variable */
  const float* presc_mask;            /* dev (B, T1, HW) mask variable */
  int mask_value, interpolate;
  const float* ar_init;               /* NULL, or dev (B, n_out, HW): a separate state to feed back into next_in instead of
                                         `gen` (use_cold_sampling_for_last_step = False hands the cold-sampled state over as
                                         "preds_autoregressive_init", stepper_multistep.py:412-418); prescribed like `gen`,
                                         the timelines still receive `gen` */
} sdy_step_finish_args;
/* prescriber + unpack into the timelines + denormalise + autoregressive feedback into next_in */
int sdy_step_finish(const sdy_step_finish_args* args, void* stream);
/* timeline slot 0: gen_norm_tl[e][b][0] = (data - mean)/std, gen_tl = that * std + mean, for the table's variables
 * (tl_norm / tl_denorm: arrays of nvars dev pointers) */
int sdy_init_timeline(const sdy_var_table* vars, int T1, int B, int HW, float* const* tl_norm, float* const* tl_denorm,
                      void* stream);
/* LpLoss.rel terms: terms[b][0] += sum (gen - target_norm)^2, terms[b][1] += sum target_norm^2 over the packed
 * (n_out, HW) fields of sample b, target_norm from `targets` at time t.  terms: dev double [B*2], zeroed by the caller. */
int sdy_lp_rel_terms(const float* gen, const sdy_var_table* targets, int t, int T1, int B, int HW, double* terms,
                     void* stream);

/* On-device ensemble diagnostics (src/ace_inference/core/metrics.py:32-54 weighted_mean, :107-132 RMSE, :135-144
 * ensemble_spread, :158-208 weighted_crps, :84-104 bias), one pass over the ensemble.
 *   pred: dev, member m of plane p at pred + m*member_stride + p*HW (M <= 64 members); truth: dev (n_planes, HW);
 *   weights: dev (HW) area weights (any normalisation: the caller divides by their sum)
 *   out[p][0..3] += sum_w (mean_m x - truth)^2 | sum_w var_m(x) (unbiased) | sum_w fair CRPS | sum_w (mean_m x - truth)
 * out: dev double [n_planes*4], zeroed by the caller. */
int sdy_ensemble_metrics(const float* pred, const float* truth, const float* weights, int M, long member_stride,
                         int n_planes, int HW, double* out, void* stream);

/* Per-timestep series terms of the reduced inference aggregator (MeanAggregator / AreaWeightedReducedMetric,
 * src/ace_inference/core/aggregator/inference/reduced.py:105-266; metrics src/ace_inference/core/metrics.py:32-208), one
 * pass over the ensemble.  Plane p = (sample s, time t), p = s*T + t:
 *   member m of plane p at pred + m*member_stride + s*sample_stride + t*HW (M <= 64; the strides let the window driver's
 *   member-stacked (members, samples, time, HW) VIEW of its device batch be read without a copy);
 *   truth plane p at truth + s*truth_sample_stride + t*HW; weights: dev (HW), any normalisation.
 *   out[p][0..7] += sum_w (mean_m x - truth)^2 | sum_w var_m(x) (unbiased) | sum_w fair CRPS | sum_w (mean_m x - truth) |
 *                   sum_w mean_m x | sum_w (mean_m x)^2 | sum_w truth | sum_w truth^2
 * out: dev double [n_sample*T*8], zeroed by the caller. */
int sdy_ensemble_series(const float* pred, int M, long member_stride, long sample_stride, const float* truth,
                        long truth_sample_stride, const float* weights, int n_sample, int T, int HW, double* out,
                        void* stream);

/* sdy_ensemble_series plus the two sums of weighted_grad_mag_percent_diff (gradient_magnitude_percent_diff,
 * src/ace_inference/core/metrics.py:210-241; fed the member-stacked prediction by reduced.py:178,225-227 and
 * one_step/reduced.py:75,121-123), in the same pass.  Planes are (nlat, nlon) rows of width nlon (HW = nlat*nlon), the
 * other arguments as for sdy_ensemble_series.  |grad x| = sqrt(g_lat^2 + g_lon^2) with torch.gradient's unit spacing and
 * edge_order 1: (x[i+1] - x[i-1]) / 2 inside, x[1] - x[0] and x[n-1] - x[n-2] at the edges, longitude NOT periodic.
 *   out[p][0..7] as sdy_ensemble_series;  out[p][8] += sum_w |grad truth|;  out[p][9] += sum_m sum_w |grad x_m|
 * (the caller divides [9] by M for the reference's mean over members).  nlat < 2 or nlon < 2: SDY_ERR_ARG (torch.gradient
 * refuses them too), as is nlat*nlon > 2^30.  out: dev double [n_sample*T*10], zeroed by the caller. */
int sdy_ensemble_series_grad(const float* pred, int M, long member_stride, long sample_stride, const float* truth,
                             long truth_sample_stride, const float* weights, int n_sample, int T, int nlat, int nlon,
                             double* out, void* stream);

/* Derived water-budget variables of the inference loop (compute_derived_quantities,
 * src/ace_inference/inference/derived_variables.py; formulas src/ace_inference/core/metrics.py:296-367), all requested
 * outputs in one pass.  Per trajectory (i0, i1) and time t, at grid point p, with q_k = specific total water of level k:
 *   dp_k  = (ak[k+1] + ps*bk[k+1]) - (ak[k] + ps*bk[k])
 *   twp   = (1/g) * sum_k dp_k*q_k                                      (total_water_path)
 *   dry   = ps - g*twp                                                  (surface_pressure_due_to_dry_air)
 *   resid = 0 at t = 0, else (twp_t - twp_{t-1}) / 21600 - (lhf/2.5e6 - prate + adv)   (total_water_path_budget_residual)
 * in the reference's fp32 operation order (no FMA contraction, levels summed in order).  The time difference is along THIS
 * time axis for every trajectory (the reference differences axis 1 of whatever it is handed, which for member-stacked
 * predictions is the sample axis).
 *   inputs: dev float, element (i0, i1, t, p) at ptr + i0*s0 + i1*s1 + t*HW + p (the window driver's member-stacked view,
 *           or flat rows with n0 = 1); q[0..K-1] and ps always; lhf, prate, adv when resid is requested
 *   outputs: dev float, contiguous (n0, n1, T, HW); each may be NULL (not computed)
 * SDY_ERR_ARG: K outside 1..SDY_DERIVED_MAX_LEVELS, a non-positive extent, HW or a stride not a multiple of 4, a required
 * input NULL, a pointer not 16-byte aligned.  SDY_ERR_UNSUPPORTED: n0*n1 > 65535. */
#define SDY_DERIVED_MAX_LEVELS 16
typedef struct {
  const float* q[SDY_DERIVED_MAX_LEVELS];
  const float* ps;
  const float* lhf;
  const float* prate;
  const float* adv;
  long s0, s1;
  int n0, n1, T, HW, K;
  float ak[SDY_DERIVED_MAX_LEVELS + 1], bk[SDY_DERIVED_MAX_LEVELS + 1];
  float* dry;
  float* twp;
  float* resid;
} sdy_derived_args;
int sdy_derived_water(const sdy_derived_args* args, void* stream);

/* Post-step state corrector of the stepper (Corrector, src/ace_inference/core/corrector.py), applied to the B samples of one
 * step: gen is the network's output, `in` the state it stepped from.  Per sample, with mean_w the area-weighted global mean
 * (metrics.weighted_mean) and dp_k / twp / dry as above, the reference's three rules in its order:
 *   SDY_CORRECTOR_DRY_AIR   err = mean_w(dry(gen)) - mean_w(dry(in));
 *                           ps  = ((dry(gen) - err) + sum_k (ak[k+1]-ak[k])*q_k) / (1 - sum_k (bk[k+1]-bk[k])*q_k)
 *   SDY_CORRECTOR_ZERO_ADV  adv -= mean_w(adv)
 *   budget (with the ps left by the first rule): tend = (twp(gen) - twp(in)) / 21600, evap = lhf / 2.5e6
 *     1 precipitation   prate *= (mean_w(evap) - mean_w(tend)) / mean_w(prate)
 *     2 evaporation     lhf    = (evap * (mean_w(tend) + mean_w(prate)) / mean_w(evap)) * 2.5e6
 *     3 / 4             1 / 2, then adv = tend - (evap - prate) per column with the corrected evap / prate
 * Elementwise arithmetic is fp32 in the reference's operation order (no FMA contraction, levels summed in order); the global
 * sums are float64 and deterministic: per-workgroup partials of fixed 1024-column chunks in the workspace, summed in chunk order
 * by one thread per sample, no atomics -- a sample's result depends neither on B, nor on its place in the batch, nor on the run.
 * Three launches whatever B, K and the flags: reduce (reads every needed plane once), solve (B threads), apply (re-reads what
 * the rewritten fields depend on).  mean_w(tend) is taken as affine in err (it is, per column, up to fp32 rounding), so the
 * apply pass needs no second reduction.  The scalars never leave the device.
 *   variable: element (b, p) at base + b*stride + channel*HW + p, physical value x*std + mean; the corrected value y is stored as
 *             (y - mean)/std with the gen variable's mean / std.  Two layouts: the stepper's packed (B, n, HW) tensors (stride =
 *             n*HW, channel = the variable's index) and plain per-variable tensors (channel 0, mean 0, std 1: exact).
 *   out_*:    where a rewritten field goes: the gen variable itself (in place) or a plane of its own; nothing else is written.
 *             out_ps with DRY_AIR, out_adv with ZERO_ADV or budget 3 / 4, out_prate with budget 1 / 3, out_lhf with 2 / 4.
 *             An out plane may be the gen variable's own plane but must not overlap any other plane that is read.
 *   area:     dev float (HW), the weights.   ws: dev, 8-byte aligned, at least the workspace bytes of (B, HW); scratch only.
 *   needed:   gen_q / in_q / gen_ps / in_ps with DRY_AIR or a budget; gen_adv with ZERO_ADV; gen_lhf / gen_prate with a budget.
 * Any HW >= 1; 16-byte loads when HW, every stride and every plane address allow it, 4-byte loads otherwise (same sums either
 * way).  A zero mean_w(prate) / mean_w(evap) or 1 - sum (bk[k+1]-bk[k])*q_k = 0 gives inf / nan as in the reference.
 * SDY_ERR_ARG, before anything is launched: NULL args / area / ws or a needed variable's base / out, B or HW < 1, K outside
 * 1..SDY_DERIVED_MAX_LEVELS when water is needed, unknown flag bits, budget outside 0..4, a negative channel or stride, with
 * B > 1 a stride below (channel+1)*HW, std not finite and > 0, mean not finite, ws misaligned or ws_bytes too small.
 * SDY_ERR_UNSUPPORTED: B > 65535.  The host twin computes the same on host memory (ws may be NULL). */
#define SDY_CORRECTOR_DRY_AIR 1
#define SDY_CORRECTOR_ZERO_ADV 2
typedef struct sdy_corrector_var {
  const float* base;
  long stride;
  int channel;
  float mean, std;
} sdy_corrector_var;
typedef struct sdy_corrector_out {
  float* base;
  long stride;
  int channel;
} sdy_corrector_out;
typedef struct sdy_corrector_args {
  int B, HW, K;
  int flags;    /* SDY_CORRECTOR_DRY_AIR | SDY_CORRECTOR_ZERO_ADV */
  int budget;   /* 0 none, 1 precipitation, 2 evaporation, 3 advection_and_precipitation, 4 advection_and_evaporation */
  float ak[SDY_DERIVED_MAX_LEVELS + 1], bk[SDY_DERIVED_MAX_LEVELS + 1];
  const float* area;
  sdy_corrector_var gen_q[SDY_DERIVED_MAX_LEVELS], in_q[SDY_DERIVED_MAX_LEVELS];
  sdy_corrector_var gen_ps, in_ps, gen_lhf, gen_prate, gen_adv;
  sdy_corrector_out out_ps, out_lhf, out_prate, out_adv;
  void* ws;
  size_t ws_bytes;
} sdy_corrector_args;
int sdy_corrector(const sdy_corrector_args* args, void* stream);
int sdy_corrector_host(const sdy_corrector_args* args);
size_t sdy_corrector_workspace_bytes(int B, int HW);

/* Dry-air conservation diagnostics (compute_dry_air_absolute_differences, src/ace_inference/core/aggregator/climate_data.py:
 * 199-233; get_dry_air_nonconservation / ConservationLoss, core/loss.py; DryAir, core/aggregator/one_step/derived.py).  For B
 * samples and T times, with dry = ps - g*twp per column as above (the fp32 chain of csrc/corrector_math.h):
 *   gm[b][t]      = sum_p area[p]*dry(b,t,p) / sum_p area[p]                 (metrics.weighted_mean over the grid)
 *   absdiff[t]    = (1/B) * sum_b |gm[b][t+1] - gm[b][t]|,  t = 0 .. T-2      (.diff(dim=-1).abs().mean(dim=0))
 *   mean_absdiff  = (1/(T-1)) * sum_t absdiff[t]                             (.mean()); with B equal rows per time this is also
 *                                                                              DryAir's mean over samples and times at once
 * all float64.  Two launches whatever B, T and K: a reduce pass that reads the K water levels, the pressure and the weights
 * once and writes one float64 partial pair per (sample, time, 1024-column chunk) to the workspace, and one small block that
 * adds the partials in chunk order, the samples in sample order and the times in time order.  No atomics: gm[b][t] depends
 * neither on B, nor on the row's place in the batch, nor on the run, and the host twin (same arithmetic, same tree inside a
 * chunk, same orders) gives the same bits.
 *   variable: element (b, t, p) at base + b*stride_b + t*stride_t + channel*HW + p, physical value x*std + mean: (B, T, H, W)
 *             dict tensors, their [:, 0:2] views and the stepper's packed (B, C, H, W) tensors (T = 1, channel = the index) all
 *             pass without a copy.
 *   area:     dev float (HW).   ak, bk: K + 1 values.
 *   gm:       dev double (B*T), always written.   absdiff: dev double (T-1).   mean_absdiff: dev double (1); with
 *             accumulate != 0 the value is ADDED to what is there (a running total over batches, in stream order).  With
 *             T = 1 neither absdiff nor mean_absdiff is touched (both may be NULL).
 *   ws:       dev, 8-byte aligned, at least sdy_dry_air_workspace_bytes(B, T, HW); scratch only.
 * SDY_ERR_ARG, before anything is launched: NULL args / area / gm / ws, with T > 1 a NULL absdiff / mean_absdiff, a NULL base
 * of ps or of one of the K levels, B, T or HW < 1, HW not a multiple of 4, K outside 1..SDY_DERIVED_MAX_LEVELS, a negative
 * channel, a negative stride or one that is not a multiple of 4, a plane address (or area) not 16-byte aligned, an output not
 * 8-byte aligned, std not finite and > 0, mean not finite, ws misaligned or ws_bytes too small.  SDY_ERR_UNSUPPORTED: B*T >
 * 65535.  The host twin computes the same on host memory (ws may be NULL). */
typedef struct sdy_dry_air_var {
  const float* base;
  long stride_b, stride_t;
  int channel;
  float mean, std;
} sdy_dry_air_var;
typedef struct sdy_dry_air_args {
  int B, T, HW, K;
  int accumulate;
  float ak[SDY_DERIVED_MAX_LEVELS + 1], bk[SDY_DERIVED_MAX_LEVELS + 1];
  const float* area;
  sdy_dry_air_var q[SDY_DERIVED_MAX_LEVELS];
  sdy_dry_air_var ps;
  double* gm;
  double* absdiff;
  double* mean_absdiff;
  void* ws;
  size_t ws_bytes;
} sdy_dry_air_args;
int sdy_dry_air_series(const sdy_dry_air_args* args, void* stream);
int sdy_dry_air_series_host(const sdy_dry_air_args* args);
size_t sdy_dry_air_workspace_bytes(int B, int T, int HW);

/* Time-mean accumulation of the inference aggregator (src/ace_inference/core/aggregator/inference/time_mean.py:97-117,
 * _add_or_initialize_time_mean): acc[p] += scale * sum over rows (r0, r1) and times t0 <= t < T of
 * x[r0*stride0 + r1*stride1 + t*HW + p].  x: dev, one variable of a window, (n0, n1, T, HW) with float strides for the
 * two leading axes (members, samples; a transposed view needs no copy); acc: dev (HW) running map.  scale = 1 / (n0 * n1 *
 * (T - t0)) gives the reference's mean over members, samples and time (t0 = 1 skips a window's initial condition).
 * HW and both strides multiples of 4, x and acc 16-byte aligned (float4 loads and stores), else SDY_ERR_ALIGN before anything
 * is launched. */
int sdy_time_mean_accumulate(const float* x, int n0, long stride0, int n1, long stride1, int t0, int T, int HW, float scale,
                             float* acc, void* stream);

/* Value histograms of the inference loop's data writer (HistogramDataWriter,
 * src/ace_inference/inference/data_writer/histograms.py; DynamicHistogram, src/ace_inference/core/histogram.py): per variable
 * and lead time, n_bins constant-width bins whose range doubles until it holds every value seen.  One call adds ONE dict (all
 * variables of the targets, or of the predictions) of one window, in three launches: min / max of every variable; the
 * reference's range rules, one workgroup per variable; counting.  Nothing is read back: range, counts and bookkeeping stay on
 * the device until the caller copies them.
 *   data[v]: dev float, element (i0, i1, t, p) of variable v at data[v] + i0*s0[v] + i1*s1[v] + t*HW + p; every (i0, i1) is a
 *            sample of lead time t_start + t (the window driver's member-stacked view, or flat rows with n0 = 1).  16-byte
 *            loads when HW, every stride and every pointer allow them, scalar loads otherwise.
 *   counts:  dev uint64 (nvars, n_times, n_bins), zeroed by the caller before the first call
 *   state:   dev, sdy_hist_state_bytes(nvars) bytes, zeroed by the caller before the first call (private layout; a host copy
 *            is read with sdy_hist_state_unpack_host)
 * Edges are never stored: edge(i) = fl32(fl32(i * step) + start), step = fl32(fl32(stop - start) / n_bins), edge(n_bins) =
 * stop -- numpy's float32 linspace, no FMA.  Bin k holds [edge(k), edge(k+1)), the last bin is closed on the right
 * (np.histogram with explicit edges).  Range rules per variable with (vmin, vmax) of THIS call: vmin == vmax widens both by
 * 1e-6 (fp32); the first call takes (vmin, vmax) as (start, stop); later, while vmin < start: start = fl32(stop - 2 *
 * fl32(stop - start)) and every time row's counts become c[2j] + c[2j+1] in the upper half; then, while vmax > stop, the
 * mirror image.  Where the reference would not terminate or would produce NaN edges -- a non-finite vmin / vmax, a zero-width
 * fp32 range (also the first range of a constant field too large for +-1e-6 to change it), a range whose step is not a
 * positive finite fp32 -- the variable's range and counts stay as they were, SDY_HIST_FLAG_RANGE is set in its sticky flags
 * word, and its values are counted as "outside".  A value outside [start, stop] or a NaN is never counted; it adds one to the
 * variable's "outside" counter (0 unless the flag is set).
 * SDY_ERR_ARG, before anything is launched: NULL args / data[v] / state / counts, nvars outside 1..SDY_MAX_VARS, a
 * non-positive n0 / n1 / T / HW / n_times, a negative stride, t_start < 0, t_start + T > n_times, n_bins odd or outside
 * 2..SDY_HIST_MAX_BINS (the counting kernel keeps 4 x n_bins words in LDS).  SDY_ERR_UNSUPPORTED: T*HW > 2^30, T > 65535. */
#define SDY_HIST_MAX_BINS 2048
#define SDY_HIST_FLAG_RANGE 1u
typedef struct sdy_hist_args {
  int nvars;
  const float* data[SDY_MAX_VARS];
  long s0[SDY_MAX_VARS], s1[SDY_MAX_VARS];
  int n0, n1, T, HW;
  int t_start, n_times, n_bins;
  void* state;
  unsigned long long* counts;
} sdy_hist_args;
int sdy_hist_add(const sdy_hist_args* args, void* stream);
size_t sdy_hist_state_bytes(int nvars);   /* 0 for nvars < 1 */
/* Variable v of a HOST copy of `state`: range, whether a first range has been taken, the sticky flags, the outside counter
 * (any output may be NULL). */
int sdy_hist_state_unpack_host(const void* state_host, int v, float* start, float* stop, int* initialised, unsigned* flags,
                               unsigned long long* outside);
/* The same arithmetic on the host (the kernels and these entry points compile one header): the range rules for one
 * (vmin, vmax) -> new range, doublings to the left and to the right, flags (SDY_HIST_FLAG_RANGE: range unchanged, 0
 * doublings); the n_bins + 1 edges of a range; the bin of each of n values (-1: outside or NaN).  Host pointers, no device. */
int sdy_hist_plan_host(float start, float stop, int initialised, float vmin, float vmax, int n_bins, float* new_start,
                       float* new_stop, int* n_left, int* n_right, unsigned* flags);
int sdy_hist_edges_host(float start, float stop, int n_bins, float* edges);
int sdy_hist_bins_host(const float* x, long n, float start, float stop, int n_bins, int* bins);

/* Time coarsening of the inference loop's data writer (TimeCoarsen,
 * src/ace_inference/inference/data_writer/time_coarsen.py:65-134): one launch for all variables of ONE dict.
 *   data[v]: dev float, element (i0, i1, t, p) of variable v at data[v] + i0*s0[v] + i1*s1[v] + t*HW + p, the in-place views
 *            sdy_hist_add takes (member-stacked (members, samples, time, lat, lon), or flat rows with n0 = 1)
 *   out[v]:  dev float, contiguous (n0, n1, T_out, HW), T_out = t_first + (T - t_first) / factor (integer division); the
 *            pointers may point into one staging buffer
 * Times t < t_first are copied unchanged (the initial condition of the first window); output time t_first + g is the mean of
 * input times t_first + g*factor .. t_first + (g+1)*factor - 1; trailing times that do not fill a group are dropped (the
 * reference's unfold(dimension=time, size=factor, step=factor).mean(-1)).  A mean is the fp32 sum of the group in time order
 * divided by factor (a true division: torch's mean is sum / count); factor == 1 is a plain gather, bit for bit.  16-byte loads
 * and stores when HW, every stride and every pointer allow them, scalar accesses otherwise.
 * SDY_ERR_ARG, before anything is launched: NULL args / data[v] / out[v], nvars outside 1..SDY_MAX_VARS, a non-positive n0 /
 * n1 / T / HW, a negative stride, factor < 1, t_first outside 0..T, T_out == 0.  SDY_ERR_UNSUPPORTED: T*HW > 2^30, n0*n1 >=
 * 2^31 (the flat work index is 64-bit: n0*n1 has no grid-dimension limit).
 * sdy_time_coarsen_host: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel
 * compiles (csrc/coarsen_mean.h), so the semantics can be pinned without a device. */
typedef struct sdy_coarsen_args {
  int nvars;
  const float* data[SDY_MAX_VARS];
  long s0[SDY_MAX_VARS], s1[SDY_MAX_VARS];
  float* out[SDY_MAX_VARS];
  int n0, n1, T, HW;
  int t_first, factor;
} sdy_coarsen_args;
int sdy_time_coarsen(const sdy_coarsen_args* args, void* stream);
int sdy_time_coarsen_host(const sdy_coarsen_args* args);

/* One window of all variables as the field aggregators below read it, in place: what the window driver hands over.
 *   gen[v]:    dev float, element (i0, i1, t, p) of variable v at gen[v] + i0*gs0 + i1*gs1 + t*plane + p: n0 members (or
 *              1), n1 samples, T times, plane = the grid points of one time (HW, or H*W; the structure that embeds the window
 *              says which).  The member-stacked (members, samples, time, lat, lon) view of the window driver is read as it
 *              is; flat rows are n0 = 1
 *   target[v]: dev float, element (i1, t, p) at target[v] + i1*ts1 + t*plane + p
 * 16-byte loads when the plane (for the zonal means: W), every stride and every pointer allow them, scalar loads otherwise
 * (same values).  Every entry point refuses, before anything is launched, with SDY_ERR_ARG: nvars outside 1..SDY_MAX_VARS, a
 * non-positive n0 / n1 / T / plane, a negative stride, a NULL gen[v] / target[v]; with SDY_ERR_UNSUPPORTED: T*plane > 2^30,
 * n0*n1 >= 2^31 (32-bit work items within a variable, 32-bit row numbers). */
typedef struct sdy_window {
  int nvars;
  const float* gen[SDY_MAX_VARS];
  const float* target[SDY_MAX_VARS];
  long gs0, gs1, ts1;
  int n0, n1, T;
} sdy_window;

/* Where the counted times of a window land in accumulators that keep one slot per lead time: embedded as `slots` in the
 * structures below that have them.
 *   t0:         the first counted time of the window: 1 when the window starts a run (its first time is the initial
 *               condition), else 0; t0 == T counts nothing: SDY_OK, nothing is launched
 *   pool_times: 0: window time t lands in slot t_start + t of n_slots; non-zero: every time lands in slot 0, n_slots must be 1
 *               and t_start is not looked at
 * Every entry point refuses, before anything is launched, with SDY_ERR_ARG: a non-positive n_slots, t0 outside 0..T; not
 * pooled: t_start < 0, t_start + T > n_slots; pooled: n_slots != 1. */
typedef struct sdy_lead_slots {
  int t0;
  int t_start, n_slots;
  int pool_times;
} sdy_lead_slots;

/* The threshold events of the variables of a call: embedded as `thr` in the structures below that test values against them.
 * Every variable of a call has the same n_events = E events.  Event e of variable v is a threshold c and a direction: a value
 * x is in the event when x > c, or (bit e of below[v] set) when x < c; both strict, a NaN x is never in it.  A point (sample,
 * time, lat, lon) is COUNTED for an event when neither its target nor its threshold is NaN; a NaN member is simply not in the
 * event.  The thresholds are device memory the caller builds once; nothing is copied per call, no address is formed from a
 * value read from device memory:
 *   scalars:   dev float, contiguous (nvars, E): the threshold of event e of variable v where bit e of is_map[v] is clear
 *              (read once per block, not per point; not looked at where the bit is set).  A NaN counts nothing.
 *   maps:      dev float, contiguous (n_maps, H*W) threshold maps; may be NULL when no is_map bit below E is set.  The map
 *              events of variable v take the planes map_first[v], map_first[v] + 1, .. in event order; a row of a map is
 *              loaded once per unit of 4 (or 1) longitudes, not once per member.
 * Every entry point refuses, before anything is launched, with SDY_ERR_ARG: n_events outside 1..SDY_EVENT_MAX, NULL scalars, a
 * map event with maps == NULL, map_first[v] < 0 or its planes past n_maps; with SDY_ERR_UNSUPPORTED: n_maps*H*W >= 2^40.  The
 * _host twins take HOST pointers.  One definition for the kernels and the _host twins: csrc/events.h. */
#define SDY_EVENT_MAX 8
typedef struct sdy_event_thresholds {
  int n_events;
  int n_maps;
  unsigned char below[SDY_MAX_VARS];
  unsigned char is_map[SDY_MAX_VARS];
  int map_first[SDY_MAX_VARS];
  const float* scalars;
  const float* maps;
} sdy_event_thresholds;

/* Per-grid-point video statistics of the inference aggregators (VideoAggregator with its extended statistics,
 * src/ace_inference/core/aggregator/inference/video.py): one launch adds ONE window of all variables to float64 accumulators
 * that stay on the device.
 *   window:    see sdy_window, plane = HW.  All n0*n1 generated rows are pooled (the reference's class takes 4-D data only:
 *              pooling members is this library's rule)
 *   accumulators: dev double, contiguous (nvars, n_timesteps, HW) each -- variable v's (n_timesteps, HW) block at
 *              base + v*n_timesteps*HW; window time t lands at time t_start + t.  gen_mean and target_mean are required; the
 *              other five are updated where their pointer is non-NULL (the caller fills err_min / err_max with +inf / -inf and
 *              the rest with 0 before the first call):
 *                gen_mean += mean over the generated rows      target_mean += mean over the target rows
 *                gen_sq, target_sq += mean of the squares
 *                err_var += UNBIASED variance over the rows of e (one row adds NaN, as torch.var of one sample)
 *                err_min = min(err_min, min over rows of e)    err_max likewise; a NaN wins, as in torch.minimum
 *              e of row (i0, i1) = fl32(gen - target row i1), the reference's single fp32 subtraction, widened to double;
 *              every sum is float64.
 * Exactly one thread owns an accumulator element (no atomics): calls that touch the same times must be ordered on a stream.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / gen_mean / target_mean, nvars outside
 * 1..SDY_MAX_VARS, a non-positive n0 / n1 / T / HW / n_timesteps, a negative stride, t_start < 0, t_start + T > n_timesteps.
 * SDY_ERR_UNSUPPORTED: T*HW > 2^30, n0*n1 >= 2^31, n_timesteps*HW >= 2^40 (flat accumulator indices are 64-bit).
 * The _host twin: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel compiles
 * (csrc/field_stats.h), so the semantics can be pinned without a device. */
typedef struct sdy_video_args {
  sdy_window win;
  int HW;
  int t_start, n_timesteps;
  double *gen_mean, *target_mean, *gen_sq, *target_sq, *err_var, *err_min, *err_max;
} sdy_video_args;
int sdy_video_accumulate(const sdy_video_args* args, void* stream);
int sdy_video_accumulate_host(const sdy_video_args* args);

/* Zonal means of the inference aggregators (ZonalMeanAggregator, .../aggregator/inference/zonal_mean.py): one launch adds ONE
 * window of all variables.  window: see sdy_window, plane = H*W.
 *   gen_acc, target_acc: dev double, contiguous (nvars, n1, n_timesteps, H) each, zeroed by the caller before the first call:
 *     gen_acc[v, s, t_start + t, lat]    += mean over the n0 members of the mean over the W longitudes of gen[v][., s, t, lat, .]
 *     target_acc[v, s, t_start + t, lat] += mean over the W longitudes of target[v][s, t, lat, .]
 *   summed in float64 (the reference sums in fp32).  The member mean is this library's rule: the reference drops the zonal
 *   mean for ensembles.  One wave per latitude row (several rows per wave when a row has fewer than 64 loads), cross-lane
 *   reduction, no atomics.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / gen_acc / target_acc, nvars outside
 * 1..SDY_MAX_VARS, a non-positive n0 / n1 / T / H / W / n_timesteps, a negative stride, t_start < 0, t_start + T >
 * n_timesteps.  SDY_ERR_UNSUPPORTED: T*H*W > 2^30, n0*n1 >= 2^31, n_timesteps*H >= 2^40, n1*n_timesteps*H >= 2^50. */
typedef struct sdy_zonal_args {
  sdy_window win;
  int H, W;
  int t_start, n_timesteps;
  double *gen_acc, *target_acc;
} sdy_zonal_args;
int sdy_zonal_accumulate(const sdy_zonal_args* args, void* stream);
int sdy_zonal_accumulate_host(const sdy_zonal_args* args);

/* Per-member time sums of an ensemble rollout (the reference's ensemble TimeMeanAggregator,
 * src/evaluation/aggregators/time_mean.py with is_ensemble=True, keeps one time-mean map per member): one launch adds ONE
 * window of all variables to float64 accumulators that stay on the device.
 *   window:     see sdy_window, plane = HW: n0 members, n1 samples
 *   t0:         the first counted time of the window: 1 when the window starts a run (its first time is the initial
 *               condition), else 0
 *   gen_sum:    dev double, contiguous (nvars, n0, n1, HW), zeroed by the caller before the first call
 *   target_sum: dev double, contiguous (nvars, n1, HW), likewise
 *     every element += the float64 sum of its fp32 values over t0 <= t < T, in ascending t
 * Exactly one thread owns an accumulator element (no atomics, no LDS): calls on the same accumulators must be ordered on a
 * stream.  The order of every sum is fixed, so an element's value is bit-identical to the _host twin's, in any batch and in
 * any run.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / gen_sum / target_sum, an accumulator not 8-byte
 * aligned, nvars outside 1..SDY_MAX_VARS, a non-positive n0 / n1 / T / HW, a negative stride, t0 outside 0..T-1.
 * SDY_ERR_UNSUPPORTED: T*HW > 2^30, n0*n1 >= 2^31, nvars*n0*n1*HW >= 2^50 (flat accumulator indices are 64-bit).
 * The _host twin: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel compiles
 * (csrc/member_mean.h), so the semantics can be pinned without a device. */
typedef struct sdy_member_sum_args {
  sdy_window win;
  int HW;
  int t0;
  double *gen_sum, *target_sum;
} sdy_member_sum_args;
int sdy_member_time_sum(const sdy_member_sum_args* args, void* stream);
int sdy_member_time_sum_host(const sdy_member_sum_args* args);

/* Area-weighted statistics of the per-member time means, all variables of one grid in one call (two launches: per-block
 * partials into ws, then the partials of a variable in block order; no atomics, bit-identical from run to run).
 *   gen_sum, target_sum: dev double, what sdy_member_time_sum accumulated: (nvars, M, n1, HW) and (nvars, n1, HW)
 *   n_times:  the number of times behind the sums; g_m = gen_sum / n_times, t = target_sum / n_times
 *   weights:  dev float (HW), widened to double
 *   out:      dev double (nvars, 2 M + 4), overwritten.  With sum_w = the sum over the n1 samples and the HW grid points of
 *             weights[p] * (.), per variable:
 *               out[m]       = sum_w (g_m - t)^2,  m < M          out[M + m]   = sum_w (g_m - t)
 *               out[2 M]     = sum_w (mean_m g - t)^2             out[2 M + 1] = sum_w (mean_m g - t)
 *               out[2 M + 2] = sum_w of the fair CRPS  mean_m |g_m - t| - sum_{i,j} |g_i - g_j| / (2 M (M - 1))
 *               out[2 M + 3] = sum_w of the unbiased variance over the members
 *             M == 1: CRPS = |g - t|, variance 0.  The caller divides by n1 * sum(weights) (after adding ranks, if any).
 *   ws:       dev, 8-byte aligned, at least sdy_member_stats_workspace_bytes(nvars, M, n1, HW); scratch only
 * Everything is float64.  The _host twin (ws may be NULL) adds the same per-point terms (csrc/member_mean.h) in the same
 * blocks of 256 points, each block in point order where the device uses a butterfly: equal to rounding, not to the bit.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen_sum / target_sum / weights / out / ws, a double pointer not 8-byte
 * aligned, a non-positive nvars / M / n1 / HW, n_times not finite and > 0, ws_bytes too small.
 * SDY_ERR_UNSUPPORTED: M > SDY_MEMBER_STATS_MAX_MEMBERS, nvars > 65535, n1*HW > 2^30, nvars*M*n1*HW >= 2^50. */
#define SDY_MEMBER_STATS_MAX_MEMBERS 64
typedef struct sdy_member_stats_args {
  int nvars, M, n1, HW;
  const double* gen_sum;
  const double* target_sum;
  const float* weights;
  double n_times;
  double* out;
  void* ws;
  size_t ws_bytes;
} sdy_member_stats_args;
int sdy_member_map_stats(const sdy_member_stats_args* args, void* stream);
int sdy_member_map_stats_host(const sdy_member_stats_args* args);
size_t sdy_member_stats_workspace_bytes(int nvars, int M, int n1, int HW);   /* 0 for arguments outside the supported range */

/* The rows of one window in the coefficient tensors of the two sides, and where their times land: embedded as `rows` in
 * sdy_spectrum_args and sdy_vector_spectrum_args below, checked by one function (csrc/coef_rows.h).  A coefficient tensor is
 * in the internal layout above as sdy_legendre_fwd / sdy_vector_legendre_fwd write it for ONE image (B = 1):
 * Cs[l][m][ri][field], m < mtr, gen_fields / target_fields fields per plane (the C of the transform, padding included).
 * Entries with m > l and fields that the decoding does not name are never read.
 *   field decoding: gen field of (variable v, member i0, sample i1, window time t) = v*gen_var_stride + t*gen_time_stride + i0*n1 + i1
 *              target field of (v, i1, t)                                     = v*target_var_stride + t*target_time_stride + i1
 *              (the rows of one (variable, time) are consecutive fields: a run of 4 x rows bytes per plane)
 *   gen_scale, target_scale: dev float [gen_fields] / [target_fields], or NULL for 1: what a field's stored coefficients are
 *              to be multiplied with, in float64 before anything else (exact for a power of two).  The split-fp16 Legendre
 *              analysis stages SDY_ACT_SX x |Xf| as fp16, so a field in physical units (a pressure in Pa) has to be handed to
 *              sdy_rfft_lon scaled down (its per-field a, with d = 0) and its scale undone here.
 *   times:     the accumulators of the embedding structure are dev double, contiguous (nvars, n_timesteps, lmax) each, zeroed
 *              by the caller before the first call; window time t < T lands at time t_start + t.
 * SDY_ERR_ARG: a non-positive lmax, mtr, field count, nvars, n0, n1, T or n_timesteps; mtr > lmax; a negative stride;
 * t_start < 0; t_start + T > n_timesteps; a buffer whose field count does not reach the last row of the last time of the last
 * variable.
 * SDY_ERR_UNSUPPORTED: n0*n1 >= 2^31 - 256 (row numbers are 32-bit), T or nvars > 65535 (grid extents), lmax*mtr*2*fields >=
 * 2^40 for either side, nvars*n_timesteps*lmax >= 2^40 (flat indices are 64-bit). */
typedef struct sdy_coef_rows {
  const float* gen_scale;
  const float* target_scale;
  int lmax, mtr;
  int gen_fields, target_fields;
  int gen_var_stride, gen_time_stride;
  int target_var_stride, target_time_stride;
  int nvars, n0, n1, T;
  int t_start, n_timesteps;
} sdy_coef_rows;            /* 72 bytes */

/* Per-degree power spectra of generated, target and error fields (no counterpart in the reference, whose only measure of
 * blurring is weighted_grad_mag_percent_diff): one launch adds ONE window of all listed variables to float64 accumulators that
 * stay on the device.  For the coefficients a[l][m] of one field (RealSHT: norm "ortho", csphase, m <= l)
 *   P(l) = |a[l,0]|^2 + 2 * sum_{m = 1 .. min(l, mtr - 1)} |a[l,m]|^2,   l < lmax
 * so that sum_l P(l) is the integral of the squared field over the sphere for a band-limited field on the Legendre-Gauss grid.
 *   gen, target: dev float, the coefficients of the two sides as sdy_legendre_fwd writes them (see sdy_coef_rows).
 *   rows:      see sdy_coef_rows: the field decoding, the scales, and where times land.
 *   accumulators: see sdy_coef_rows.  gen_power and target_power are required, err_power may be NULL:
 *                gen_power    += mean over the n0*n1 generated rows of P of the row
 *                target_power += mean over the n1 target rows of P of the row
 *                err_power    += mean over the n0*n1 rows of P of (gen row (i0, i1) - target row i1), from the coefficient
 *                                differences (the transform is linear), the two fp32 coefficients subtracted in float64
 *              The cross spectrum sum_m w_m Re(gen conj(target)), pooled likewise, is (gen_power + target_power - err_power)/2.
 * Every sum is float64 in a fixed order (csrc/spectrum.h): a row's orders in ascending m; the rows of an element in 256 slots
 * (row r in slot r % 256, ascending r) that meet in a butterfly.  One wave owns an accumulator element: no atomics, no LDS;
 * calls that touch the same times must be ordered on a stream.  A row's P(l) depends on its own coefficients only, whatever
 * else the call holds; device and host twin give the same bits.  16-byte loads of a buffer whose pointer is 16-byte aligned
 * and whose field count and two strides are multiples of 4; 4-byte loads otherwise (same values).
 * SDY_ERR_ARG, before anything is launched: NULL args / gen / target / gen_power / target_power; what sdy_coef_rows refuses.
 * SDY_ERR_UNSUPPORTED: what sdy_coef_rows refuses.
 * The _host twin: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel compiles
 * (csrc/spectrum.h), so the semantics can be pinned without a device. */
typedef struct sdy_spectrum_args {
  const float* gen;
  const float* target;
  sdy_coef_rows rows;
  double *gen_power, *target_power, *err_power;
} sdy_spectrum_args;
int sdy_degree_power(const sdy_spectrum_args* args, void* stream);
int sdy_degree_power_host(const sdy_spectrum_args* args);

/* Rotational and divergent kinetic-energy spectra of a horizontal wind (no counterpart in the reference; the definition is the
 * library's own).  A wind with eastward component u and northward component v has the tangent components
 * V_theta = -v (colatitude) and V_lambda = u.  In the orthonormal vector harmonics Psi = grad Y / sqrt(l (l + 1)) and
 * Phi = r x grad Y / sqrt(l (l + 1)), with A_T[f](l, m) = sum_k w_k T[m][l][k] f_m(k) the Legendre analysis by a table T of what
 * sdy_rfft_lon delivers:
 *   s(l,m) = A_D[V_theta] - i A_M[V_lambda]     spheroidal: the divergent part
 *   t(l,m) = A_D[V_lambda] + i A_M[V_theta]     toroidal: the rotational part
 *   E_div(l) = 1/2 (|s(l,0)|^2 + 2 sum_{m = 1 .. min(l, mtr - 1)} |s(l,m)|^2),   E_rot(l) the same of t,   l < lmax
 * so that sum_l (E_rot + E_div) = 1/2 integral of (u^2 + v^2) over the unit sphere for a band-limited wind on the
 * Legendre-Gauss grid (not an identity on the equiangular grid with lmax = nlat); units (wind unit)^2 sr.
 *
 * The two tables, host-only and fp64, [mmax][lmax][nlat] each (P the table of sdy_sht_tables_host, norm "ortho", csphase), both
 * divided by sqrt(l (l + 1)) with row l = 0 identically zero:
 *   dtab = dP_l^m / dtheta in the ladder form, finite at the poles:
 *          m >= 1: 1/2 [sqrt((l-m)(l+m+1)) P_l^{m+1} - sqrt((l+m)(l-m+1)) P_l^{m-1}],   m = 0: sqrt(l (l+1)) P_l^1
 *   mtab = m P_l^m / sin(theta); at the two pole nodes of the equiangular grid its limit: 0 for m != 1, and
 *          sign(cos theta) dP_l^1 / dtheta for m = 1.
 * SDY_ERR_ARG for a NULL table, nlat or nlon < 2, lmax or mmax < 1 or an unknown grid.  No GPU needed. */
int sdy_vsht_tables_host(int nlat, int nlon, int lmax, int mmax, int grid, double* dtab, double* mtab);

/* The vector plan of an existing plan: the two tables above, quadrature-weighted, in fp32 on the device in the layout of the
 * scalar analysis table ([mtr][nlat][lmax rounded up to 4]).  It owns nothing else -- the longitude FFT is the base plan's --
 * and refers to the base plan, which must outlive it.  SDY_ERR_ARG for a NULL argument. */
typedef struct sdy_vsht_plan sdy_vsht_plan;
int sdy_vsht_plan_create(const sdy_sht_plan* plan, sdy_vsht_plan** out);
void sdy_vsht_plan_destroy(sdy_vsht_plan* vplan);
/* Vector Legendre analysis of Xf as sdy_rfft_lon of the base plan writes it: Cs_d = A_D and Cs_m = A_M of every field, in the
 * layout and with the exact zeros (m > l) of sdy_legendre_fwd.  Both products run on the fp32 batched MFMA GEMM, whatever the
 * base plan's gemm_mode: the derivative table has the opposite equatorial parity to the scalar table, so the folded
 * split-fp16 kernels cannot take it as it is.  Cs_d and Cs_m must not overlap.  SDY_ERR_ARG for a NULL pointer or B, C < 1;
 * SDY_ERR_ALIGN for an odd C. */
int sdy_vector_legendre_fwd(const sdy_vsht_plan* vplan, const float* Xf, float* Cs_d, float* Cs_m, int B, int C, void* stream);

/* One launch adds ONE window of all listed wind pairs to float64 accumulators that stay on the device.
 *   struct_size: sizeof of this structure.  It stands in for the sdy_abi_check handshake, whose list this structure is not
 *              part of: a call with another value is refused (SDY_ERR_ARG).  The size did not change when `rows` replaced
 *              the loose fields (168 bytes before and after, but the v offsets moved from bytes 72 / 76 to 112 / 116 and the
 *              ten integers behind them up by 8), so struct_size does NOT tell a caller compiled against the earlier header
 *              from a current one: recompile C callers with this header.
 *   gen_d, gen_m, target_d, target_m: dev float, Cs_d and Cs_m of sdy_vector_legendre_fwd for ONE image per side.  The u rows
 *              and the v rows of a side are two runs of one field batch: the field decoding of sdy_coef_rows names the u
 *              field of a row (nvars counts pairs), and its v field lies gen_v_offset / target_v_offset fields further.
 *   rows:      see sdy_coef_rows; gen_scale and target_scale per field (u and v fields have their own).
 *   accumulators: dev double, contiguous (nvars, n_timesteps, lmax) each.  gen_rot, gen_div, target_rot, target_div are
 *              required; err_rot and err_div are both given or both NULL.  Each adds the mean over the rows of E_rot / E_div
 *              of the row; the error of generated row (i0, i1) is taken of s_gen - s_target and t_gen - t_target against
 *              target row i1.
 * Per row and order the eight fp32 values (re / im of A_D[u], A_D[v], A_M[u], A_M[v]) are multiplied by their field's scale in
 * float64, combined into s and t, and the m-weight times their squared moduli is added, orders ascending; rows meet as in
 * sdy_degree_power (csrc/vector_spectrum.h, csrc/spectrum.h).  Device and host twin give the same bits.  16-byte loads where
 * the two pointers of a side are 16-byte aligned and its field count, v offset and two strides are multiples of 4 (a group's
 * last quad of fields is then loaded whole and the fields past its last row are discarded: they lie inside the plane).
 * SDY_ERR_ARG, before anything is launched: NULL args, another struct_size, a NULL coefficient tensor or required
 * accumulator, one error accumulator without the other; what sdy_coef_rows refuses; a negative v offset or one that carries the
 * last row past its buffer.  SDY_ERR_UNSUPPORTED: what sdy_coef_rows refuses.  The _host twin takes HOST pointers. */
typedef struct sdy_vector_spectrum_args sdy_vector_spectrum_args;
struct sdy_vector_spectrum_args {
  size_t struct_size;
  const float *gen_d, *gen_m, *target_d, *target_m;
  sdy_coef_rows rows;
  int gen_v_offset, target_v_offset;
  double *gen_rot, *gen_div, *target_rot, *target_div, *err_rot, *err_div;
};
int sdy_vector_degree_power(const sdy_vector_spectrum_args* args, void* stream);
int sdy_vector_degree_power_host(const sdy_vector_spectrum_args* args);

/* Relative vorticity, divergence, streamfunction and velocity potential of winds (no counterpart in the reference; the
 * definition is the library's own): the coefficients of up to four scalar fields per wind from the
 * products of the vector Legendre analysis, ready for the scalar synthesis.  With s and t as above (V = sum s Psi + t Phi) and
 * the wind on a sphere of radius a written V = grad chi + r x grad psi (u = -d psi/dy + d chi/dx, v = d psi/dx + d chi/dy, so
 * that zeta = laplace psi and delta = laplace chi), in the convention of sdy_sht_inverse:
 *   psi(l,m) = a t(l,m) / sqrt(l (l + 1))      chi(l,m)   = a s(l,m) / sqrt(l (l + 1))
 *   zeta(l,m) = -sqrt(l (l + 1)) t(l,m) / a    delta(l,m) = -sqrt(l (l + 1)) s(l,m) / a          all four zero at l = 0
 * Solid-body rotation u = U cos(lat), v = 0 gives zeta = 2 U sin(lat) / a and psi = -a U sin(lat).
 *
 * sdy_helmholtz_factors_host: host-only, one row out[lmax] of the factor table: kind 0 is -sqrt(l (l + 1)) / radius (zeta,
 * delta), kind 1 is radius / sqrt(l (l + 1)) (psi, chi); out[0] = 0, and out[l] = 0 for l > truncate when truncate >= 0 (a
 * triangular truncation is a property of the table).  SDY_ERR_ARG for a NULL out, lmax < 1, a radius that is not finite and
 * positive, or another kind.
 *
 * sdy_helmholtz_coefficients: one launch.
 *   struct_size: sizeof of this structure (it is not part of the sdy_abi_check list; another value is refused).
 *   Cs_d, Cs_m: dev float, what sdy_vector_legendre_fwd writes for ONE image (B = 1): [lmax][mtr][ri][fields].  The u fields are
 *              the n_winds fields from u_offset, the v fields the n_winds fields from v_offset.  Entries with m > l and fields
 *              outside the two runs are never read, except the fields that complete a run's last quad.
 *   scale:     dev float [fields] or NULL for 1: what a field's stored coefficients are multiplied with, as in sdy_coef_rows.
 *   factor:    dev double [n_out][lmax].
 *   out:       dev float [lmax][mtr][ri][out_fields], for sdy_legendre_inv with B = 1, C = out_fields.  Output q < n_out of wind
 *              i is field q * out_stride + i; it is part[q] (0: s, 1: t) with both components multiplied by factor[q][l] in
 *              float64 and rounded once to fp32.  Exact zeros: row l = 0, entries with m > l, and every field no output names.
 *              out must not overlap Cs_d or Cs_m.
 * The arithmetic is csrc/helmholtz.h and csrc/vector_spectrum.h; a wind's values depend on its own eight coefficients only;
 * device and host twin give the same bits.
 * SDY_ERR_ARG, before anything is launched: NULL args / Cs_d / Cs_m / factor / out, another struct_size, n_out outside 1..4, a
 * part outside {0, 1}, a non-positive lmax, mtr, fields, out_fields or n_winds, a negative offset or stride, a run or an output
 * plane that leaves its tensor, planes closer than n_winds rounded up to four, out overlapping an input.
 * SDY_ERR_ALIGN: fields, out_fields, u_offset, v_offset or out_stride not a multiple of 4; Cs_d, Cs_m, scale or out not
 * 16-byte aligned, factor not 8-byte aligned.  SDY_ERR_UNSUPPORTED: 2^31 or more quads of fields in one call.
 * The _host twin takes HOST pointers. */
typedef struct sdy_helmholtz_args sdy_helmholtz_args;
struct sdy_helmholtz_args {
  size_t struct_size;
  const float *Cs_d, *Cs_m;
  const float* scale;
  const double* factor;
  float* out;
  int lmax, mtr;
  int fields, u_offset, v_offset, n_winds;
  int out_fields, out_stride, n_out;
  int part[4];
};
int sdy_helmholtz_factors_host(int lmax, double radius, int kind, int truncate, double* out);
int sdy_helmholtz_coefficients(const sdy_helmholtz_args* args, void* stream);
int sdy_helmholtz_coefficients_host(const sdy_helmholtz_args* args);

/* Per-trajectory time variance and lag-1 autocorrelation at every grid point (no counterpart in the reference): the second
 * moments along time of a rollout, kept on the device.  A trajectory is a member of a sample, or a sample's target.  For its
 * counted times x_1 .. x_n (fp32) at one grid point, in run order (csrc/variability.h):
 *   c = x_1 (fp32),  d_t = (double)x_t - (double)c,  S1 = sum d_t,  S2 = sum d_t d_t,  P = sum_{t >= 2} d_{t-1} d_t,
 *   last = x_n (fp32).  S1, S2, P are float64; every time's term is added to the running value in ascending time, so the bits
 *   do not depend on how a run is cut into windows.  The shift by the first value keeps the variance of a field with a large
 *   mean (surface pressure) to float64 rounding of the deviations.
 * One launch adds ONE window of all variables to the state:
 *   window:      see sdy_window, plane = HW: n0 members, n1 samples
 *   t0:          the first counted time of the window: 1 when the window starts a run (its first time is the initial
 *                condition), else 0
 *   first:       non-zero for the first counted window of a run: the state is not read, c = x[t0] and x[t0] has no predecessor;
 *                zero: the predecessor of x[t0] is the state's `last`
 *   s1, s2, p:   dev double, contiguous (nvars, n0*n1 + n1, HW) each: row i0*n1 + i1 is member i0 of sample i1, rows n0*n1 + i1
 *                are the targets
 *   origin_last: dev float, contiguous (nvars, n0*n1 + n1, HW, 2): the pair (c, last), 8-byte aligned
 * Exactly one thread owns a state element (no atomics, no LDS): calls on the same state must be ordered on a stream.  The order
 * of every sum is fixed, so the state is bit-identical to the _host twin's, in any layout, batch and run.  16-byte loads (and
 * 32-byte accesses of the state) when the window allows them and the state pointers are 32-byte aligned, scalar otherwise.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / s1 / s2 / p / origin_last, a state pointer not
 * 8-byte aligned, nvars outside 1..SDY_MAX_VARS, a non-positive n0 / n1 / T / HW, a negative stride, t0 outside 0..T-1.
 * SDY_ERR_UNSUPPORTED: T*HW > 2^30, n0*n1 >= 2^31, nvars*(n0+1)*n1*HW >= 2^50 (flat state indices are 64-bit).
 * The _host twin: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel compiles
 * (csrc/variability.h), so the semantics can be pinned without a device. */
typedef struct sdy_variability_args {
  sdy_window win;
  int HW;
  int t0;
  int first;
  double *s1, *s2, *p;
  float* origin_last;
} sdy_variability_args;
int sdy_time_variability_accumulate(const sdy_variability_args* args, void* stream);
int sdy_time_variability_accumulate_host(const sdy_variability_args* args);

/* The state after n_times counted times -> variance and lag-1 autocorrelation, elementwise over n_elems state elements:
 *   m = S1 / n,  V = max(S2 - S1 m, 0),  variance = V / n (population),
 *   C = P - m ((S1 - d_n) + S1) + (n - 1) m m  with d_n = (double)last - (double)c  (the lag-1 covariance sum; d_1 = 0),
 *   lag1 = C / V where n >= 2 and V > 0, NaN otherwise.  A NaN in the state gives NaN in both.
 *   variance, lag1: dev double (n_elems), overwritten.  Device and _host twin give the same bits.
 * SDY_ERR_ARG: NULL args or pointer, a pointer not 8-byte aligned, n_elems < 1, n_times not finite and >= 1.
 * SDY_ERR_UNSUPPORTED: n_elems >= 2^39. */
typedef struct sdy_variability_maps_args {
  long n_elems;
  const double *s1, *s2, *p;
  const float* origin_last;
  double n_times;
  double *variance, *lag1;
} sdy_variability_maps_args;
int sdy_time_variability_maps(const sdy_variability_maps_args* args, void* stream);
int sdy_time_variability_maps_host(const sdy_variability_maps_args* args);

/* Area-weighted sums of the maps above, all variables of one grid in one call (two launches: per-block partials into ws, then
 * the partials of a variable in block order; no atomics, bit-identical from run to run).
 *   s1, s2, p, origin_last: the state of M members and n1 samples, (nvars, M*n1 + n1, HW) as above;  n_times: counted times
 *   weights:  dev float (HW), widened to double
 *   out:      dev double (nvars, 6), overwritten.  With sum_w = the sum over the n1 samples and the HW grid points of
 *             weights[p] * (.), per variable:
 *               out[0] = sum_w mean_m variance_gen            out[1] = sum_w variance_target
 *               out[2] = sum_w (mean_m sqrt(variance_gen) - sqrt(variance_target))^2
 *               over the points where n_times >= 2 and the target and every member have V > 0:
 *               out[3] = sum_w mean_m lag1_gen    out[4] = sum_w lag1_target    out[5] = sum_w
 *             The caller divides by n1 * sum(weights), or by out[5] (after adding ranks, if any).
 *   ws:       dev, 8-byte aligned, at least sdy_time_variability_workspace_bytes of (nvars, n1, HW); scratch only
 * Everything is float64.  The _host twin (ws may be NULL) adds the same per-point terms (csrc/variability.h) in the same blocks
 * of 256 points, each block in point order where the device uses a butterfly: equal to rounding, not to the bit.
 * SDY_ERR_ARG, before anything is launched: NULL args / s1 / s2 / p / origin_last / weights / out / ws, a state pointer, out or
 * ws not 8-byte aligned, a non-positive nvars / M / n1 / HW, n_times not finite and >= 1, ws_bytes too small.
 * SDY_ERR_UNSUPPORTED: nvars > 65535, n1*HW > 2^30, nvars*(M+1)*n1*HW >= 2^50. */
typedef struct sdy_variability_stats_args {
  int nvars, M, n1, HW;
  const double *s1, *s2, *p;
  const float* origin_last;
  const float* weights;
  double n_times;
  double* out;
  void* ws;
  size_t ws_bytes;
} sdy_variability_stats_args;
int sdy_time_variability_stats(const sdy_variability_stats_args* args, void* stream);
int sdy_time_variability_stats_host(const sdy_variability_stats_args* args);
size_t sdy_time_variability_workspace_bytes(int nvars, int n1, int HW);   /* 0 for a non-positive argument */

/* Regional area-weighted metric sums (MeanAggregator's eight sums of sdy_ensemble_series, once per region): ONE launch for all
 * variables and all regions of one window; the member and target values of a grid point are loaded once, whatever n_regions.
 *   window:    see sdy_window, plane = HW: n0 = M members (1 for a deterministic run), n1 samples
 *   weights:   dev float, contiguous (n_regions, HW): area weight x the region's fraction of the cell, finite and >= 0
 *   out:       dev double, contiguous (nvars, n_regions, n1, T, 8), WRITTEN (not accumulated):
 *                out[v][r][s][t][q] = sum over the grid points i of weights[r][i] * q_i,  q in the order of sdy_ensemble_series:
 *                (em - y)^2 | unbiased member variance | fair CRPS | em - y | em | em^2 | y | y^2
 *              with y the target and em the ensemble mean of the point.  M == 1: CRPS = |g - y|, variance 0.  The caller
 *              divides by the sum of the region's weights.
 *   ws:        dev, 8-byte aligned, at least sdy_region_series_workspace_bytes of (nvars, n_regions, n1, T, HW); scratch only
 * Per-point arithmetic (csrc/region_series.h, compiled by the kernel and by the _host twin): float64 throughout and nothing
 * contracted; em - y = mean_m (g_m - y) and em = y + (em - y): the deviations are taken from the differences to y, which are
 * exact in float64 for fp32 inputs.
 * ZERO-WEIGHT RULE: a point whose weight in a region is exactly 0 contributes NOTHING to that region, whatever its values,
 * NaN and inf included (IEEE's 0 x NaN = NaN is deliberately not followed: an ocean-only field with NaN over land gives finite
 * sums for a region that is zero over land).  Anywhere else a NaN propagates into the sums it belongs to.
 * Order of the sums: a plane is cut into chunks of 1024 consecutive grid points (a rule of HW alone); a chunk's four quarters
 * of 256 points are summed one by one and added in ascending order, the chunks' partials go to ws and are added in ascending
 * order by a second launch: no atomics, and the 8 * n_regions sums of a plane depend on that plane and the weights only -- the
 * same bits in any batch, layout (16-byte or scalar loads) and run.  The _host twin adds a quarter's points in point order
 * where the device adds lane-strided partial sums over a wave: equal to the rounding of a float64 sum, not to the bit.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / weights / out / ws, out or ws not 8-byte aligned,
 * nvars outside 1..SDY_MAX_VARS, n_regions outside 1..SDY_REGION_MAX, a non-positive n0 / n1 / T / HW, a negative stride,
 * ws_bytes too small.  SDY_ERR_UNSUPPORTED: n0 > SDY_REGION_MAX_MEMBERS, T*HW > 2^30, n0*n1 >= 2^31, more than 2^31 - 1
 * (sample, time, chunk) work items per variable, nvars*n_regions*n1*T*8 >= 2^38 (the grid of the second launch).
 * The _host twin: the same structure with HOST pointers and the same checks (ws may be NULL). */
#define SDY_REGION_MAX 16
#define SDY_REGION_MAX_MEMBERS 64
typedef struct sdy_region_series_args {
  sdy_window win;
  int HW;
  int n_regions;
  const float* weights;
  double* out;
  void* ws;
  size_t ws_bytes;
} sdy_region_series_args;
int sdy_region_series(const sdy_region_series_args* args, void* stream);
int sdy_region_series_host(const sdy_region_series_args* args);
size_t sdy_region_series_workspace_bytes(int nvars, int n_regions, int n1, int T, int HW);   /* 0 for an argument out of range */

/* Threshold events of an ensemble: the counts behind Brier score, reliability diagram, ROC curve and exceedance-frequency maps
 * (no counterpart in the reference).  window: see sdy_window, plane = H*W: n0 = M members, n1 samples.  slots: see
 * sdy_lead_slots.  thresholds: see sdy_event_thresholds.  Per counted point k = the number of members in the event (0 .. M)
 * and o = 1 if the target is in it, else 0.  Integers only.
 * sdy_event_table_accumulate:  acc = table, dev double, contiguous (nvars, n_slots, E, H, 2, M + 1), zeroed by the caller:
 *   table[v, slot, e, lat, o, k] += the counted points of the row's W longitudes, n1 samples (and, pooled, T - t0 times) with
 *   that (o, k).  One group of lanes owns the accumulator row (v, slot, lat): its E x 2 x (M + 1) bins are 32-bit words in LDS
 *   (integer LDS atomics) that the owner adds to the accumulators with plain load / add / store; every member value is loaded
 *   once and tested against all E thresholds.  The rows of a block are capped so that its LDS stays within 64 KB.
 * sdy_event_frequency_accumulate:  acc = maps, dev double, contiguous (nvars, E, 3, H*W), zeroed by the caller:
 *   acc[v, e, 0, p] += sum of k, acc[v, e, 1, p] += sum of o, acc[v, e, 2, p] += the counted points, over the n1 samples and
 *   the T - t0 counted times of grid point p.  One thread owns a grid point (four with 16-byte loads), sums in integer
 *   registers and touches the accumulator once.  All lead times are pooled: t_start / n_slots / pool_times are checked as for
 *   the table and otherwise not used.
 * No global atomics, no second pass; calls on the same accumulators must be ordered on a stream.  Every count is bit-identical
 * to the _host twin's, in any layout, batch and run.  16-byte loads when W, every stride and every pointer (maps included)
 * allow them.
 * SDY_ERR_ARG, before anything is launched: what sdy_window, sdy_lead_slots and sdy_event_thresholds refuse; NULL args / acc,
 * acc not 8-byte aligned, a non-positive H / W.
 * SDY_ERR_UNSUPPORTED: what sdy_event_thresholds refuses; n0 > SDY_EVENT_MAX_MEMBERS; table: the points of one row in one call
 * (n1*W, pooled: n1*W*T) >= 2^32 (the row's 32-bit words), n_slots*H >= 2^40, nvars*n_slots*E*H*2*(n0+1) >= 2^50, one row's
 * bins over 64 KB of LDS; frequency: n0*n1*T >= 2^31 (the 32-bit registers of a point), nvars*E*3*H*W >= 2^50.
 * The _host twins: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernels
 * compile (csrc/events.h). */
#define SDY_EVENT_MAX_MEMBERS 64
typedef struct sdy_event_args {
  sdy_window win;
  int H, W;
  sdy_lead_slots slots;
  sdy_event_thresholds thr;
  double* acc;
} sdy_event_args;
int sdy_event_table_accumulate(const sdy_event_args* args, void* stream);
int sdy_event_table_accumulate_host(const sdy_event_args* args);
int sdy_event_frequency_accumulate(const sdy_event_args* args, void* stream);
int sdy_event_frequency_accumulate_host(const sdy_event_args* args);

/* Neighbourhood verification of threshold events: the integer sums behind the fractions skill score (no counterpart in the
 * reference).  window: see sdy_window, plane = H*W: n0 = M members, n1 samples.  slots: see sdy_lead_slots.  thresholds: see
 * sdy_event_thresholds.  One definition for the kernels and the _host twin: csrc/fss.h (integers and comparisons only).
 * Per (variable v, sample s, time t, event e) and grid point q: c(q) = 1 when q is counted, else 0; k(q) = the members in the
 * event, o(q) = 1 when the target is in it; k = o = 0 where c = 0.  The neighbourhood of radius r >= 0 of a centre (lat, lon):
 * the points (lat', (lon + d) mod W) with |lat' - lat| <= r, 0 <= lat' < H and |d| <= r -- longitude wraps, latitude is clipped
 * at the poles; measured in grid points, not kilometres.  n(lat, r) = (2r + 1) (min(H - 1, lat + r) - max(0, lat - r) + 1).
 * K, O, C = the sums of k, o, c over the neighbourhood.  A centre is COUNTED when C = n(lat, r): every point of its
 * neighbourhood is counted (a NaN target or a NaN in a threshold map removes the centres within r of it; it is never read as
 * "not in the event").
 *   radii:    n_radii (1 .. SDY_FSS_MAX_RADII) radii, strictly ascending, 0 allowed, 2r + 1 <= W
 *   acc:      dev double, contiguous (nvars, n_slots, E, n_radii, H, 6), zeroed by the caller, holding integers:
 *             acc[v, slot, e, j, lat, :] += (count, sum K, sum O, sum K^2, sum K O, sum O^2) over the counted centres of radius
 *             radii[j] among the row's W longitudes, the n1 samples and, pooled, the T - t0 counted times
 *   ws:       dev, 8-byte aligned, at least sdy_fss_workspace_bytes(nvars, E, n1, T, H, W); scratch only
 * Two launches.  sdy_fss_encode reads the window once, in place, tests every member value against all E thresholds of its
 * point and writes one 16-bit code per (v, s, t, e, point) to ws: k in bits 0-6, o in bit 7, c in bit 8.  sdy_fss_sum: a block
 * owns the accumulator rows of one (v, slot, e) and one band of latitudes; per radius, sample and counted time it forms in LDS
 * the horizontal periodic sums of the band's rows and r halo rows, then the vertical clipped sums, adds the six terms of every
 * counted centre to 64-bit integer row sums and, at the end, each row sum to acc once with a plain load / add / store.  No
 * global atomics; no address is formed from a value read from memory; calls on the same accumulators or workspace must be
 * ordered on a stream.  sdy_fss_accumulate is the two in order.  Every sum is an integer: the same bits in any layout, batch,
 * band size, grouping of variables and run, and equal to the _host twin's.  One call's sums are exact (checked below); across
 * calls the float64 accumulators are exact below 2^53 and round above it: not checked.
 * SDY_ERR_ARG, before anything is launched: what sdy_window, sdy_lead_slots and sdy_event_thresholds refuse; NULL args / acc /
 * ws, acc or ws not 8-byte aligned, a non-positive H / W;
 * n_radii outside 1..SDY_FSS_MAX_RADII, a negative radius, radii not strictly ascending, 2r + 1 > W; ws_bytes too small.
 * SDY_ERR_UNSUPPORTED: n0 > SDY_EVENT_MAX_MEMBERS; n0 (2 r_max + 1)^2 > 65535 (K fits 16 bits, K^2 32); what
 * sdy_event_thresholds refuses; the
 * largest row sum of one call, n1 W (pooled: x (T - t0)) (n0 n_max)^2 with n_max = (2 r_max + 1) min(H, 2 r_max + 1), >= 2^53;
 * n_slots*H >= 2^40, nvars*n_slots*E*n_radii*H*6 or the codes of the workspace >= 2^50; 2 r_max + 1 rows of W 32-bit sums and
 * one of W + 2 r_max over 64 KB of LDS; more than 2^24 - 1 (counted time, band of latitudes) blocks per variable and event.
 * The _host twin: the same structure with HOST pointers and the same checks (ws may be NULL). */
#define SDY_FSS_MAX_RADII 4
typedef struct sdy_fss_args {
  sdy_window win;
  int H, W;
  sdy_lead_slots slots;
  sdy_event_thresholds thr;
  int n_radii;
  int radii[SDY_FSS_MAX_RADII];
  double* acc;
  void* ws;
  size_t ws_bytes;
} sdy_fss_args;
int sdy_fss_accumulate(const sdy_fss_args* args, void* stream);
int sdy_fss_accumulate_host(const sdy_fss_args* args);
int sdy_fss_encode(const sdy_fss_args* args, void* stream);   /* the first launch of sdy_fss_accumulate alone */
int sdy_fss_sum(const sdy_fss_args* args, void* stream);      /* the second: ws holds the codes of sdy_fss_encode of the same args */
size_t sdy_fss_workspace_bytes(int nvars, int n_events, int n1, int T, int H, int W);   /* 0 for an argument out of range */

/* Spell durations of threshold events: how long an event lasts along a trajectory -- consecutive dry days, warm spells (no
 * counterpart in the reference).  window: see sdy_window, plane = H*W: n0 = M members, n1 samples.  thresholds: see
 * sdy_event_thresholds.  One definition for the kernel and the _host twin: csrc/spells.h (integers and comparisons only).
 *   struct_size: sizeof of this structure.  It stands in for the sdy_abi_check handshake, whose list this structure is not
 *              part of: a call with another value is refused (SDY_ERR_ARG).
 * A trajectory is one member of one sample, or one sample's target, at one grid point: row r of rows = n0*n1 + n1, the
 * generated ones first (member r / n1, sample r % n1), then the targets.  Its counted times are the window times t0 .. T - 1
 * of every call, in call order; t0 == T is SDY_OK and launches nothing.  A value is in event e as sdy_event_thresholds says; a
 * NaN
 * value never is, for the target too, so it ends a spell.  A spell is a maximal run of consecutive counted times in the event.
 *   state:     dev, 32-bit unsigned words, contiguous (nvars, E, 4, rows, H*W), 8-byte aligned, zeroed by the caller before
 *              the first window and carried from call to call: word 0 = run, the length of the spell open after the last
 *              counted time (0 when that time was outside the event); 1 = longest, the maximum run has reached; 2 = spells,
 *              the spells begun; 3 = hits, the counted times in the event.  Read and written once per call.
 *   durations: dev double, contiguous (nvars, E, 2, H, 16), zeroed by the caller: durations[v, e, side, lat, bin] += the spells
 *              of length d that END in this call at latitude lat, pooled over the longitudes and the generated (side 0) or
 *              target (side 1) trajectories; bin = the number of edges 1, 2, 4, .., 16384 below d, at most 15.  A spell ends
 *              at the first counted time outside the event after it; one that is still open is in `run` only, so state and
 *              durations have the same bits however a run is cut into calls.
 * A grid point whose threshold is NaN is in no event: its state stays zero and it adds nothing; what to report there is the
 * caller's.  One block owns the accumulator row (v, lat): every (trajectory, 4 longitudes) of it is a work item of one lane,
 * which loads its thresholds and state once, keeps the window's times in flight, tests every value once against all E
 * thresholds and stores the state once; the row's E x 2 x 16 bins are 32-bit words in LDS (integer LDS atomics) that are added
 * to durations with plain load / add / store.  No global atomics, no second pass; calls on the same state must be ordered on a
 * stream.  Bit-identical to the _host twin.  16-byte accesses when W, every stride and every pointer (maps and state included)
 * allow them.
 * SDY_ERR_ARG, before anything is launched: what sdy_window and sdy_event_thresholds refuse; NULL args, another struct_size,
 * NULL state / durations, state or durations not 8-byte aligned, a non-positive H / W, t0 outside 0..T.
 * SDY_ERR_UNSUPPORTED: what sdy_event_thresholds refuses; n0 > SDY_EVENT_MAX_MEMBERS; (n0*n1 + n1)*W*T >= 2^32 (a row's 32-bit
 * LDS words) or
 * (n0*n1 + n1)*W > 2^32 - 256 (its 32-bit work items);
 * nvars*E*4*rows*H*W or nvars*E*2*H*16 >= 2^50.
 * The _host twin: the same structure with HOST pointers and the same checks. */
#define SDY_SPELL_BINS 16
typedef struct sdy_event_spell_args sdy_event_spell_args;
struct sdy_event_spell_args {
  size_t struct_size;
  sdy_window win;
  int H, W;
  int t0;
  sdy_event_thresholds thr;
  unsigned* state;
  double* durations;
};
int sdy_event_spell_accumulate(const sdy_event_spell_args* args, void* stream);
int sdy_event_spell_accumulate_host(const sdy_event_spell_args* args);

/* Per-grid-point quantiles along time of gen and target, exactly (no counterpart in the reference): the trajectories of a run
 * kept as sortable 32-bit keys, and any set of quantiles selected out of them without sorting.  One definition for the kernels
 * and the _host twins: csrc/quantile.h.  Both structures carry struct_size (sizeof of the structure; a call with another value
 * is refused with SDY_ERR_ARG) and are not part of the sdy_abi_check list.
 *   Key of an fp32 value x: -0.0 is taken as +0.0; with u the bits of x the key is u ^ 0x80000000 when the sign bit is clear
 *     and ~u when it is set, so the unsigned order of keys is the order of values, -inf first and +inf last.  Every NaN has the
 *     key 0xFFFFFFFF, which is also the "nothing recorded here" fill of a series.  The inverse gives x back bit for bit.
 *   Trajectories: rows as for the spells above -- the n0*n1 generated ones (member r / n1, sample r % n1), then the n1
 *     targets: n_traj = n0*n1 + n1, or the n1 targets alone (row = sample) when store_gen == 0.
 *   series: dev, 32-bit unsigned keys, contiguous (nvars, n_traj, capacity, H*W), 4-byte aligned, filled with 0xFFFFFFFF by the
 *     caller before the first window.
 * append: window: see sdy_window, plane = H*W.  Writes the keys of the window times t0 .. T - 1 of every trajectory to
 *   series[v][trajectory][slot0 + (t - t0)][point]; t0 == T is SDY_OK and launches nothing.  A strided copy with the key
 *   transform: (variable, trajectory) is one contiguous run of (T - t0)*H*W values on both sides.  16-byte accesses when H*W,
 *   every stride and every pointer (series included) allow them, 4-byte ones otherwise (same keys).
 *   SDY_ERR_ARG, before anything is launched: what sdy_window refuses; NULL args, another struct_size, a NULL or misaligned
 *   series, a non-positive H / W / capacity, t0 outside 0..T, slot0 < 0, slot0 + (T - t0) > capacity, store_gen not 0 or 1.
 *   SDY_ERR_UNSUPPORTED: nvars*n_traj*capacity*H*W >= 2^50.
 * select: ONE variable block (n_traj, capacity, plane) of a series.  Group g of n_groups pools the trajectories first + g*step
 *   + i*stride, i < count, over the time slots 0 .. n_slots - 1: gen pooled over members per sample is first 0, step 1, count
 *   M, stride n1, n_groups n1; gen per member count 1, n_groups M*n1; the targets first M*n1, count 1, n_groups n1.  The values
 *   of a group at a point are its keys that are not the NaN key (nanquantile semantics); n is their number, written to
 *   valid[group][point] (int).  out[group][i][point] (double) is the quantile q[i], NaN when n == 0.  Rank rule, all float64 with
 *   contraction off: h = q*(n - 1); j = min(floor(h), n - 1); g = h - j; lo the j-th smallest value (0-based), hi the min(j + 1,
 *   n - 1)-th.  method 1 (lower): lo.  2 (higher): hi when g > 0, else lo.  0 (linear): lo when g == 0 or lo == hi; otherwise,
 *   with d = hi - lo, hi - d*(1 - g) when g >= 0.5, else lo + d*g.  lower and higher are always exactly an fp32 value of the
 *   input.  Selection by 2-bit digits, most significant first: a lane owns a grid point (or 4 with 16-byte loads), counts per
 *   pass the keys that share a rank's decided prefix and have the next digit below 1, 2 and 3, and fixes the digit; one more
 *   pass settles hi.  At most 4 quantiles per launch (more are taken in two launches).  No sort, no scratch copy, no atomics.
 *   SDY_ERR_ARG, before anything is launched: NULL args, another struct_size, NULL or misaligned series / out / valid, a
 *   non-positive plane / n_traj / capacity / n_slots / count / n_groups, n_slots > capacity, a negative first / step / stride, a
 *   group's trajectory past n_traj, nq outside 1..SDY_MAX_QUANTILES, a q outside [0, 1] or NaN, method outside 0..2.
 *   SDY_ERR_UNSUPPORTED: plane > 2^30, count*n_slots >= 2^31 (32-bit counts), n_traj*capacity*plane or n_groups*nq*plane >= 2^50.
 * Both are bit-identical to their _host twins (the same structures with HOST pointers and the same checks). */
#define SDY_MAX_QUANTILES 8
typedef struct sdy_time_quantile_append_args sdy_time_quantile_append_args;
struct sdy_time_quantile_append_args {
  size_t struct_size;
  sdy_window win;
  int H, W;
  int t0;
  int slot0;
  int capacity;
  int store_gen;
  unsigned* series;
};
int sdy_time_quantile_append(const sdy_time_quantile_append_args* args, void* stream);
int sdy_time_quantile_append_host(const sdy_time_quantile_append_args* args);
typedef struct sdy_time_quantile_select_args sdy_time_quantile_select_args;
struct sdy_time_quantile_select_args {
  size_t struct_size;
  const unsigned* series;
  long plane;
  int n_traj, capacity, n_slots;
  int first, step, count, stride, n_groups;
  int nq, method;
  double q[SDY_MAX_QUANTILES];
  double* out;
  int* valid;
};
int sdy_time_quantile_select(const sdy_time_quantile_select_args* args, void* stream);
int sdy_time_quantile_select_host(const sdy_time_quantile_select_args* args);

/* Wavenumber-frequency (Wheeler-Kiladis) power of a field in an equatorial band, gen and target, on the device (no counterpart in
 * the reference).  Two entry points: append turns the band rows of a window's times into zonal Fourier coefficients of their
 * parts symmetric and antisymmetric about the equator and stores them in a ring of N time slots; segment_power turns the N
 * stored times of one segment into power per frequency and adds it to the accumulators.  One definition for the kernels and the
 * _host twins: csrc/spacetime.h.  Everything after the fp32 loads is float64, never contracted to FMA; every value is one
 * sequential chain in ascending index order; no libm call: the tables come from the caller.  Both structures carry struct_size
 * (a call with another value is refused with SDY_ERR_ARG) and are not part of the sdy_abi_check list.
 *   Trajectories: as for sdy_time_quantile_append: the n0*n1 generated ones (member r / n1, sample r % n1), then the n1 targets:
 *     n_traj = n0*n1 + n1.
 *   coef: dev double, contiguous (nvars, n_traj, N, R, 2, K + 1, 2): slot, pair, fold (0 symmetric, 1 antisymmetric),
 *     wavenumber, (re, im).
 * append: window: see sdy_window, plane = H*W.  Pair p reads the rows north[p] and south[p] (equal for an equator row).  For a
 *   window time t in t0 .. t1 - 1 (t0 == t1: SDY_OK, nothing is launched) and longitude j, in float64: s = (x_N + x_S) * 0.5, a =
 *   (x_N - x_S) * 0.5; for fold y in (s, a) and k = 0 .. K, with i = (k*j) mod W and (cos, sin) = lon_table[2 i], [2 i + 1]:
 *     re <- re + y*cos, im <- im - y*sin, j ascending from 0.0; stored re / W, im / W
 *   in slot (n_first + (t - t0)) mod N.  lon_table: dev double, W pairs (cos(2 pi i / W), sin(2 pi i / W)).  A block stages a pair's
 *   two rows in LDS and a thread owns one (fold, k) chain.  16-byte loads when W, every stride and every pointer allow them, 4-byte
 *   ones otherwise (same bits).
 *   SDY_ERR_ARG, before anything is launched: what sdy_window refuses; NULL args, another struct_size, a NULL lon_table or coef
 *   or one not 8-byte aligned, a non-positive H / W / R, K outside 0..W/2, a row index outside 0..H-1, t0 or t1 outside 0..T, t1 <
 *   t0, t1 - t0 > N, n_first < 0, N outside 4..SDY_ST_MAX_SEGMENT.
 *   SDY_ERR_UNSUPPORTED: R > SDY_ST_MAX_PAIRS, W > SDY_ST_MAX_LON (the rows' LDS), n_first >= 2^50, nvars*n_traj*N*R*2*(K+1)*2 >= 2^50.
 * segment_power: the segment whose first counted time sits in slot first_slot; its time n is slot (first_slot + n) mod N.  Per
 *   column (variable, trajectory, pair, fold, k), re and im alike, with d_n = n - (N - 1) / 2:
 *     detrend 0: z~_n = z_n;  1: z~_n = z_n - mean;  2: z~_n = (z_n - mean) - d_n * slope, mean = (sum_n z_n) / N, slope =
 *     (sum_n d_n z_n) / (sum_n d_n d_n);  y_n = z~_n * taper[n]
 *     X_f = sum_n y_n (cos u - i sin u), u from time_table[(f n) mod N]: re <- (re + y_re*cos) + y_im*sin, im <- (im + y_im*cos)
 *     - y_re*sin, n ascending from 0.0;  P_f = (re*re + im*im) / (N * sum_n taper[n]^2)
 *   acc[v][side][sample][fold][f][k] (dev double, contiguous (nvars, 2, B, 2, N, K + 1), side 0 gen and 1 target) <- acc + S,
 *   S the chain from 0.0 over (member ascending, pair ascending; the target has one member) of P_f.  taper: dev double, N values;
 *   time_table: dev double, N pairs (cos(2 pi i / N), sin(2 pi i / N)).  A block stages the N values of a tile of wavenumbers of
 *   one (variable, trajectory, pair, fold) in LDS and a thread owns frequencies; the P of every column go to ws and a second
 *   launch adds them in the order above (sdy_sum_chunks, csrc/ordered_sum.h): no atomics, the same bits in any layout, batch and
 *   run.  A non-finite coefficient makes every frequency of its column, and so of its accumulator cells, NaN.
 *   SDY_ERR_ARG, before anything is launched: NULL args, another struct_size, a NULL coef / taper / time_table / acc / ws or
 *   one not 8-byte aligned, a non-positive nvars / M / B / R, K < 0, N outside 4..SDY_ST_MAX_SEGMENT, first_slot outside
 *   0..N-1, detrend outside 0..2, ws_bytes below sdy_spacetime_workspace_bytes.
 *   SDY_ERR_UNSUPPORTED: nvars*(M*B + B)*N*R*2*(K+1)*2 >= 2^50 or more than 2^31 - 1 blocks.
 * Both are bit-identical to their _host twins (the same structures with HOST pointers and the same checks; ws may be NULL). */
#define SDY_ST_MAX_PAIRS 128
#define SDY_ST_MAX_LON 4096
#define SDY_ST_MAX_SEGMENT 1024
typedef struct sdy_spacetime_append_args sdy_spacetime_append_args;
struct sdy_spacetime_append_args {
  size_t struct_size;
  sdy_window win;
  int H, W;
  int R;
  int north[SDY_ST_MAX_PAIRS], south[SDY_ST_MAX_PAIRS];
  int K;
  const double* lon_table;
  int t0, t1;
  long n_first;
  int N;
  double* coef;
};
int sdy_spacetime_append(const sdy_spacetime_append_args* args, void* stream);
int sdy_spacetime_append_host(const sdy_spacetime_append_args* args);
typedef struct sdy_spacetime_segment_power_args sdy_spacetime_segment_power_args;
struct sdy_spacetime_segment_power_args {
  size_t struct_size;
  const double* coef;
  int nvars, M, B;
  int N, R, K;
  int first_slot;
  int detrend;
  const double* taper;
  const double* time_table;
  double* acc;
  void* ws;
  size_t ws_bytes;
};
int sdy_spacetime_segment_power(const sdy_spacetime_segment_power_args* args, void* stream);
int sdy_spacetime_segment_power_host(const sdy_spacetime_segment_power_args* args);
size_t sdy_spacetime_workspace_bytes(int nvars, int M, int B, int N, int R, int K);   /* 0 for an argument out of range */

/* Transient-eddy covariances of groups of variables at every grid point, on the device (no counterpart in the reference): the
 * second moments along time of two variables together -- the momentum flux u'v', the heat flux v'T', the moisture flux v'q',
 * the eddy kinetic energy, the correlation of any two variables at a point.  One definition for the kernels and the _host
 * twins: csrc/time_covariance.h.  The three structures carry struct_size (sizeof of the structure; a call with another value is
 * refused with SDY_ERR_ARG) and are not part of the sdy_abi_check list.
 *   A group is an ordered set of K variables, 2 <= K <= SDY_TC_MAX_K, on one grid; NP = K (K + 1) / 2 pairs i <= j in the order
 *     (0,0), (0,1), .., (0,K-1), (1,1), ..
 *   One trajectory at one grid point, counted times x_k,1 .. x_k,n (fp32) in run order: c_k = x_k,1, d_k,t = (double)x_k,t -
 *     (double)c_k, S_k = sum_t d_k,t, P_ij = sum_t d_i,t d_j,t.  float64, every product rounded once, every time's term added to
 *     the running value in ascending time: the bits do not depend on how a run is cut into windows.
 *   Trajectories: rows as for the time variability above -- the n0*n1 generated ones (member r / n1, sample r % n1), then the n1
 *     targets: rows = n0*n1 + n1.
 *   sums: dev double (n_groups, K, rows, HW); products: dev double (n_groups, NP, rows, HW); origins: dev float (n_groups, K,
 *     rows, HW), the c_k.  K + NP float64 and K fp32 per group, trajectory and point: 128 bytes at K = 4.
 * accumulate: ONE launch for all groups of one K.  window: see sdy_window, plane = HW, over the unique variables of the call;
 *   members[g][k] is the window variable that is variable k of group g.  Adds the window times t0 .. T - 1; first != 0: the run's
 *   first counted time is t0, the state is written without being read.  Every input value of a group is read once per window,
 *   the state is read and written once, exactly one thread owns a state element: no atomics, no LDS.  16-byte loads and 32-byte
 *   state accesses when HW, every stride and every pointer allow them, scalar ones otherwise (same bits).
 *   SDY_ERR_ARG, before anything is launched: what sdy_window refuses; NULL args, another struct_size, K outside
 *   2..SDY_TC_MAX_K, n_groups outside 1..SDY_TC_MAX_GROUPS, a member index outside 0..nvars-1 or repeated within a group, NULL
 *   sums / products / origins, sums or products not 8-byte aligned, origins not 4-byte aligned, t0 outside 0..T-1.
 *   SDY_ERR_UNSUPPORTED: n_groups*NP*rows*HW >= 2^50.
 * maps: ONE group and one pair i <= j < K: sums and products are the group's blocks (K, n_elems) and (NP, n_elems), n_elems =
 *   rows*HW.  With n = n_times, m_k = S_k / n, C_ij = P_ij - S_i m_j (the lower index as S), V_k = C_kk clamped at 0 (a NaN stays
 *   one): cov[e] = C_ij / n (i == j: V_i / n), corr[e] = C_ij / sqrt(V_i V_j) clamped to [-1, 1], NaN unless n >= 2, V_i > 0 and
 *   V_j > 0.  cov, corr: dev double (n_elems).  One thread per element.
 *   SDY_ERR_ARG: NULL args, another struct_size, a NULL or misaligned pointer, K outside 2..SDY_TC_MAX_K, i or j outside 0..K-1,
 *   i > j, n_elems < 1, n_times below 1 or not finite.  SDY_ERR_UNSUPPORTED: NP*n_elems >= 2^50 or more than 2^31 - 1 blocks.
 * stats: all pairs of the n_groups groups of one K -> out (n_groups, NP, SDY_TC_SLOTS), per pair the sums over the n1 samples
 *   and the HW grid points, with w = weights[p], g_m the M members and y the target of the sample:
 *     slot 0: w mean_m cov(g_m)   1: w cov(y)   2: w (mean_m cov(g_m) - cov(y))^2
 *     and over the points where n >= 2 and corr(y) and every corr(g_m) are not NaN:
 *     slot 3: w mean_m corr(g_m)  4: w corr(y)  5: w
 *   Chunks of 256 points: a wave's lanes by a butterfly, the waves in order, then the chunks in order (csrc/ordered_sum.h).
 *   weights: dev float (HW); ws: dev, 8-byte aligned, at least sdy_time_covariance_workspace_bytes of (K, n_groups, n1, HW).
 *   SDY_ERR_ARG: NULL args, another struct_size, a NULL or misaligned pointer, K outside 2..SDY_TC_MAX_K, n_groups outside
 *   1..SDY_TC_MAX_GROUPS, a non-positive M / n1 / HW, n_times below 1 or not finite, ws_bytes too small.  SDY_ERR_UNSUPPORTED:
 *   n1*HW > 2^30, n_groups*NP*(M + 1)*n1*HW >= 2^50.
 * State and maps are bit-identical to their _host twins (the same structures with HOST pointers and the same checks; ws may be
 * NULL); the stats _host twin uses the same chunks and adds a chunk's points in order. */
#define SDY_TC_MAX_K 4
#define SDY_TC_MAX_GROUPS 32
#define SDY_TC_SLOTS 6
typedef struct sdy_time_covariance_args sdy_time_covariance_args;
struct sdy_time_covariance_args {
  size_t struct_size;
  sdy_window win;
  int HW;
  int t0;
  int first;
  int K, n_groups;
  int members[SDY_TC_MAX_GROUPS][SDY_TC_MAX_K];
  double* sums;
  double* products;
  float* origins;
};
int sdy_time_covariance_accumulate(const sdy_time_covariance_args* args, void* stream);
int sdy_time_covariance_accumulate_host(const sdy_time_covariance_args* args);
typedef struct sdy_time_covariance_maps_args sdy_time_covariance_maps_args;
struct sdy_time_covariance_maps_args {
  size_t struct_size;
  const double* sums;
  const double* products;
  int K, i, j;
  long n_elems;
  double n_times;
  double* cov;
  double* corr;
};
int sdy_time_covariance_maps(const sdy_time_covariance_maps_args* args, void* stream);
int sdy_time_covariance_maps_host(const sdy_time_covariance_maps_args* args);
typedef struct sdy_time_covariance_stats_args sdy_time_covariance_stats_args;
struct sdy_time_covariance_stats_args {
  size_t struct_size;
  int K, n_groups;
  int M, n1, HW;
  const double* sums;
  const double* products;
  const float* weights;
  double n_times;
  double* out;
  void* ws;
  size_t ws_bytes;
};
int sdy_time_covariance_stats(const sdy_time_covariance_stats_args* args, void* stream);
int sdy_time_covariance_stats_host(const sdy_time_covariance_stats_args* args);
size_t sdy_time_covariance_workspace_bytes(int K, int n_groups, int n1, int HW);   /* 0 for an argument out of range */

/* Time sums and extremes per time bin (no counterpart in the reference): a window's times belong to different bins -- the
 * months, seasons or years of a calendar, the hours of the day -- and every bin keeps its own float64 sum and, optionally,
 * its fp32 maximum and minimum, per variable, trajectory and grid point, on the device.  One launch adds ONE window of a run of
 * same-shaped variables.  One definition for the kernel and the _host twin: csrc/time_bins.h.  The structure carries
 * struct_size (sizeof of the structure; a call with another value is refused with SDY_ERR_ARG) and is not part of the
 * sdy_abi_check list.
 *   window:     see sdy_window, plane = HW: n0 members, n1 samples
 *   groups:     the counted times of the call, grouped by bin: group g is the bin group_bin[g] and the window times
 *               times[group_end[g - 1]] .. times[group_end[g] - 1] (group_end[-1] = 0), ascending; every bin at most once,
 *               every time at most once, at most SDY_BIN_MAX_TIMES times per call (the caller cuts a longer window into
 *               calls, in time order).  n_groups == 0: nothing is counted, SDY_OK, nothing is launched.
 *   Accumulators: a bin's block holds bin_vars >= nvars variables, of which this call's are the first nvars (the caller offsets
 *               the pointers to the call's first variable): the element of (bin b, variable v, row r, point p) is at
 *               ((b * bin_vars + v) * rows + r) * HW + p, so that one bin of a run of variables is the contiguous (bin_vars,
 *               members, samples, HW) block that sdy_member_map_stats takes.
 *   gen_sum:    dev double (n_bins, bin_vars, n0, n1, HW), row r = member * n1 + sample; pool_members != 0: (n_bins, bin_vars, 1,
 *               n1, HW), the members of a sample added into one element.  Zeroed by the caller before the first call
 *   target_sum: dev double (n_bins, bin_vars, n1, HW), likewise
 *   gen_max, gen_min, target_max, target_min: dev float of the same shapes, all four or none; filled with -inf (max) and +inf
 *               (min) by the caller before the first call: what an empty bin keeps
 * CHAIN ORDER.  The sum of one (bin, element) is ONE sequential float64 chain acc = acc + (double)x over its counted times in
 * the order given (run order, when the caller lists them so); pooled: the members in member order inside each time.  The
 * accumulator is loaded, the group's values are added to it one by one, and it is stored: there is no per-window partial sum
 * (sdy_member_time_sum folds one and is therefore not invariant).  Every bit is the same however a run is cut into windows and
 * calls, in any layout (16-byte or scalar loads) and batch, in any order of the groups (bins are independent chains), and
 * equal to the _host twin's.
 * EXTREMES.  max: kept = x when x > kept or x is NaN, min likewise with <: a NaN makes the extreme of that bin and element NaN
 * from then on (no later value compares above or below it).
 * Exactly one thread owns an accumulator element (no atomics, no LDS): calls on the same accumulators must be ordered on a
 * stream.  An accumulator element is read and written once per group of the call, every input value is read once.
 * SDY_ERR_ARG, before anything is launched: what sdy_window refuses; NULL args, another struct_size, HW < 1, n_bins < 1,
 * bin_vars < nvars, n_groups outside 0..SDY_BIN_MAX_TIMES, a bin outside 0..n_bins-1 or listed twice, a group_end that does
 * not exceed the one before (an empty group) or exceeds SDY_BIN_MAX_TIMES, a time outside 0..T-1 or listed twice, the times of
 * a group not ascending, NULL gen_sum / target_sum, a sum not 8-byte aligned, one extreme pointer without the others, an
 * extreme not 4-byte aligned.
 * SDY_ERR_UNSUPPORTED: n_bins*bin_vars*(n0 + 1)*n1*HW >= 2^50 (flat accumulator indices are 64-bit).
 * The _host twin: the same structure with HOST pointers and the same checks. */
#define SDY_BIN_MAX_TIMES 64
typedef struct sdy_binned_sum_args sdy_binned_sum_args;
struct sdy_binned_sum_args {
  size_t struct_size;
  sdy_window win;
  int HW;
  int n_bins, bin_vars;
  int pool_members;
  int n_groups;
  int group_bin[SDY_BIN_MAX_TIMES];
  unsigned short group_end[SDY_BIN_MAX_TIMES];
  unsigned short times[SDY_BIN_MAX_TIMES];
  double *gen_sum, *target_sum;
  float *gen_max, *gen_min, *target_max, *target_min;
};
int sdy_binned_time_accumulate(const sdy_binned_sum_args* args, void* stream);
int sdy_binned_time_accumulate_host(const sdy_binned_sum_args* args);

/* The area-weighted Gram matrix of the member errors and the truth anomaly (no counterpart in the reference): what the energy
 * score, the member-to-member and member-to-truth distances of whole fields and the anomaly correlation are read from.  ONE
 * launch for all variables of one window.  window: see sdy_window, plane = HW: n0 = M members (1 for a deterministic run), n1
 * samples.  For one (variable v, sample s, time t), with g_m the members, y the target, w the weights and c the climatology,
 * N = M + 2 float64 vectors over the grid points p:
 *   a_0(p) = 1      a_{1+m}(p) = (double)g_m(p) - (double)y(p)      a_{M+1}(p) = (double)y(p) - (double)c(p)
 *   Gamma[i][j] = sum_p w(p) a_i(p) a_j(p),  0 <= i <= j < N
 * The differences are exact in float64; the errors, not the fields, enter, so that a squared distance Gamma_ii + Gamma_jj -
 * 2 Gamma_ij does not cancel the field's own magnitude.
 *   weights:     dev float, contiguous (HW): area weights, finite and >= 0, not normalised (Gamma[0][0] is their sum)
 *   climatology: per variable dev float, contiguous (HW), or NULL: c = 0 (the same bits as a map of zeros)
 *   out:         dev double, contiguous (nvars, n1, T, N (N + 1) / 2), WRITTEN: the packed upper triangle, row-major in (i, j >=
 *                i): entry (i, j) at i N - i (i - 1) / 2 + (j - i) (sdy_gram_index, csrc/member_gram.h)
 *   ws:          dev, 8-byte aligned, at least sdy_member_gram_workspace_bytes of (nvars, n0, n1, T, HW); scratch only
 * ZERO-WEIGHT RULE: a point with w(p) == 0 contributes NOTHING, NaN and inf included: every a_i of that point reads as 0, it
 * is not multiplied by 0.  Anywhere else a NaN propagates into every entry it touches and into no other: a NaN in member m
 * poisons the entries with index 1 + m (its row and its column).
 * Order of the sums: a plane is cut into chunks of 1024 consecutive grid points (a rule of HW alone) and a chunk into four
 * quarters of 256; wave k of a block takes points 64 k .. 64 k + 63 of every quarter, four points per v_mfma_f64_16x16x4_f64 in
 * ascending order, into one accumulator per entry; a chunk is wave 0 + wave 1 + wave 2 + wave 3, a plane its chunks in
 * ascending order (a second launch): no atomics, and the entries of a plane depend on that plane, the weights and the
 * climatology only -- the same bits in any batch, layout (16-byte or scalar loads), grouping of variables and run.  The _host
 * twin follows the same partition with plain loops; the order in which the instruction adds its four products is its own:
 * equal to the rounding of a float64 sum (|error| <= (HW + 4) 2^-53 sum_p w |a_i a_j| for either), not to the bit.
 * SDY_ERR_ARG, before anything is launched: what sdy_window refuses; NULL args / weights / out / ws, weights or a climatology
 * not 4-byte aligned, out or ws not 8-byte aligned, HW < 1, ws_bytes too small.
 * SDY_ERR_UNSUPPORTED: n0 > SDY_GRAM_MAX_MEMBERS, more than 2^31 - 1 (sample, time, chunk) work items per variable,
 * nvars*n1*T*N(N+1)/2 >= 2^38 (the grid of the second launch; flat ws indices then stay below 2^50).
 * The _host twin: the same structure with HOST pointers and the same checks (ws may be NULL). */
#define SDY_GRAM_MAX_MEMBERS 64
typedef struct sdy_member_gram_args {
  sdy_window win;
  int HW;
  const float* weights;
  const float* climatology[SDY_MAX_VARS];
  double* out;
  void* ws;
  size_t ws_bytes;
} sdy_member_gram_args;
int sdy_member_gram(const sdy_member_gram_args* args, void* stream);
int sdy_member_gram_host(const sdy_member_gram_args* args);
size_t sdy_member_gram_workspace_bytes(int nvars, int n0, int n1, int T, int HW);   /* 0 for an argument out of range */

/* Rank (Talagrand) histograms of an ensemble per latitude (no counterpart in the reference): one launch adds ONE window of all
 * variables to float64 accumulators that stay on the device.  window: see sdy_window, plane = H*W: n0 = M members, n1 samples.
 * For the target y and the members g_0 .. g_{M-1} of a grid point (variable v, sample s, window time t, lat, lon):
 *   rank = #{m : g_m < y}, 0 .. M.  A point whose target is NaN is counted nowhere; a NaN member is not below (the comparison
 *   is false).  The point is a tie when y is not NaN and some g_m == y; ties do not change the rank and are counted apart.
 *   slots:      see sdy_lead_slots
 *   counts:     dev double, contiguous (nvars, n_slots, H, M + 1), zeroed by the caller before the first call:
 *                 counts[v, slot, lat, rank] += the counted points of the row's W longitudes, n1 samples (and, pooled, T - t0
 *                 times) with that rank
 *   ties:       dev double, contiguous (nvars, n_slots, H), likewise: += the ties among the same points
 * One group of lanes owns an accumulator row (v, slot, lat): the row's bins are 32-bit words in LDS (integer LDS atomics)
 * that the owner adds to the accumulators with plain load / add / store: no global atomics, no second pass; calls on the same
 * accumulators must be ordered on a stream.  Integers below 2^53 add exactly in any order: every count is bit-identical to
 * the _host twin's, in any layout, batch and run.  16-byte loads when W, every stride and every pointer allow them.
 * SDY_ERR_ARG, before anything is launched: NULL args / gen[v] / target[v] / counts / ties, an accumulator not 8-byte aligned,
 * nvars outside 1..SDY_MAX_VARS, a non-positive n0 / n1 / T / H / W, a negative stride; what sdy_lead_slots refuses.
 * SDY_ERR_UNSUPPORTED: n0 > SDY_RANK_HIST_MAX_MEMBERS, T*H*W > 2^30, n0*n1 >= 2^31, the points of one row in one call (n1*W,
 * pooled: n1*W*T) >= 2^32 (the row's 32-bit words), n_slots*H >= 2^40, nvars*n_slots*H*(n0+1) >= 2^50 (flat accumulator
 * indices are 64-bit).
 * The _host twin: the same structure with HOST pointers and the same checks; the arithmetic is the header the kernel compiles
 * (csrc/rank_hist.h), so the semantics can be pinned without a device. */
#define SDY_RANK_HIST_MAX_MEMBERS 64
typedef struct sdy_rank_hist_args {
  sdy_window win;
  int H, W;
  sdy_lead_slots slots;
  double *counts, *ties;
} sdy_rank_hist_args;
int sdy_rank_hist_accumulate(const sdy_rank_hist_args* args, void* stream);
int sdy_rank_hist_accumulate_host(const sdy_rank_hist_args* args);

/* ---------------------------------------------------------------------------------------------------------
 * Sticky status word of the CURRENT device.  Kernels only ever set bits; the host reads (and optionally clears) it once per
 * window, not per launch (MultiStepStepper.run_on_batch does, after the window's single loss read-back).
 *   SDY_FLAG_NONFINITE  an InstanceNorm statistic (sum or sum of squares over H x W) came out inf / NaN: the tensor feeding
 *                       that norm holds non-finite values.
 *   SDY_FLAG_F16_RANGE  a split-precision ("h3") kernel was handed an activation with |value * scale| >= 65504, the fp16
 *                       range of its hi part (scale is 16 for the convolutions and the MLP): the products turn into inf / NaN.
 *                       The fp32-MFMA mode (gemm_mode 0, SDY_GEMM_MODE=f32) has no such limit.
 * sdy_status_flags synchronises `stream` before reading. */
#define SDY_FLAG_NONFINITE 1u
#define SDY_FLAG_F16_RANGE 2u
int sdy_status_flags(unsigned* flags, int reset, void* stream);
/* The same without the synchronisation: the word is copied to `flags_host` (pinned host memory) when `stream` reaches the
 * call, and cleared behind the copy if `reset`; read it after an event recorded behind the call has completed (the window
 * driver reads a window's word, together with its loss terms, while the next window computes). */
int sdy_status_flags_async(unsigned* flags_host, int reset, void* stream);
/* Range headroom (debug read-back; first contact with a trained checkpoint should report "x N below the cliff", not pass /
 * fail).  While enabled (process-wide switch; off by default: the bookkeeping is one atomic per tile), the split-precision
 * kernels of the default path record the largest magnitude they stage as fp16 -- pre-scale included, i.e. the number that
 * must stay below 65504 -- per consumer class, on the current device:
 *   [0] conv_h3 (inner skip and the other Cin -> 256 convolutions)   [1] mlp_h3's x tile   [2] dh_h3's coefficient rows
 *   [3] Legendre analysis input, recorded where it is PRODUCED (rfft360's stores; the folded kernel adds the two hemispheres'
 *       entries, so the recorded value is 2 x 16 x |Xf|)   [4] Legendre synthesis input, recorded at dh_h3's stores (16 x |Cs|).
 * The folded Legendre kernel has no register to spare for a tracker of its own: the two producers raise SDY_FLAG_F16_RANGE
 * for it (rfft360 at 2 x 16 x |Xf| >= 65504 -- conservative by at most the factor 2 of the fold).
 * sdy_range_headroom copies the five values (0 where a class has not run), clears them if `reset`, and synchronises `stream`.
 * headroom factor = 65504 / value. */
#define SDY_RANGE_SLOTS 5
int sdy_range_headroom_enable(int on);
int sdy_range_headroom(float* max_staged5, int reset, void* stream);
/* The dropout stream's generator evaluated on the host by the library itself (the same function the kernels inline):
 * the number of Philox rounds it was built with (7; tests hold it to oracle/philox.py and to Random123's seven-round
 * known-answer vectors) and the four words of one counter / key pair. */
int sdy_dropout_stream_rounds(void);
int sdy_dropout_stream_words(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t key_lo, uint32_t key_hi,
                             uint32_t* out4);
/* The forward-conditioning noise stream (above) written out: out dev (B, C, HW) receives eps of row b = trajectory
 * batch_offset + b % n, call + b / n (n = rows_per_call, 0 means B), channel c, pixel p -- what sdy_sfno_forward draws for a
 * generated group of C channels.  HW % 4 == 0 and out 16-byte aligned (float4 stores), else SDY_ERR_ALIGN. */
int sdy_cond_noise_fill(uint64_t seed, uint32_t call, uint32_t batch_offset, int rows_per_call, int B, int C, int HW, float* out,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Measurement.  While enabled, every kernel launch of sdy_sfno_forward is bracketed by a pair of
 * hipEvents recorded ON THE LAUNCH STREAM, tagged with its stage (fused MLP with / without dropout, inner-skip conv,
 * Legendre analysis / synthesis, rfft, irfft, dhconv, encoder / decoder convs, ...).  sdy_profile_read synchronises
 * those events, returns per stage the summed elapsed milliseconds and the launch count since the last read, and resets.
 * Not for timed regions: the extra event records add a few microseconds between kernels.  Process-wide switch. */
int sdy_profile_enable(int on);
int sdy_profile_stage_count(void);
const char* sdy_profile_stage_name(int stage);
int sdy_profile_read(double* total_ms, long* launches, int n);   /* arrays of n >= sdy_profile_stage_count() */
/* The same, plus per stage the summed batch rows its launches worked on (rows / launches = average batch of a launch: with
 * the drop-path skip a block's kernels run on the trajectories its DropPath draw keeps). */
int sdy_profile_read_rows(double* total_ms, long* launches, long* rows, int n);

/* ---------------------------------------------------------------------------------------------------------
 * Relay hand-over between processes by SDMA copy (ensemble.RelayComm(transport="peer")).  The sender
 * copies a relayed trajectory's state into a slot of a pool it has exported; the receiver maps the pool once and pulls the
 * slot into its own memory.  Neither side launches a kernel or enqueues anything that waits for the other process.
 *   sdy_relay_pool_create   one hipMalloc of n_slots x slot_bytes (dev), rounded up to 2 MiB, and the 64-byte IPC handle of
 *                           the whole allocation (hipIpcGetMemHandle on its base: never a suballocation).  Allocates.
 *   sdy_relay_pool_destroy  hipFree of the pool (synchronises the device).  Only once every process that opened the pool
 *                           has closed its mapping: a mapping left open onto freed memory faults on its next access.
 *   sdy_ipc_open / close    hipIpcOpenMemHandle (hipIpcMemLazyEnablePeerAccess) / hipIpcCloseMemHandle of another
 *                           process's handle; works between two processes on one device as well as across devices.
 *   sdy_copy_nocu           hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDeviceNoCU, stream): enqueued on the copy
 *                           engines, no compute unit used. */
int sdy_relay_pool_create(size_t slot_bytes, int n_slots, void** base, unsigned char handle[64]);
int sdy_relay_pool_destroy(void* base);
int sdy_ipc_open(const unsigned char handle[64], void** ptr);
int sdy_ipc_close(void* ptr);
int sdy_copy_nocu(void* dst, const void* src, size_t bytes, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SDY_AMD_H */
