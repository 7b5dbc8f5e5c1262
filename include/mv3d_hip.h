/* mv3d_hip.h -- C ABI of libmv3d_hip.so: the MI355X (gfx950) kernels behind the
 * appearance-flow train step of aclike/dynamic_multiview_3d.
 *
 * The reference has no native code: every entry point below replaces one TensorFlow-1.3
 * op call site of dyn_mult_view/mv3d/utils/tf_utils.py (cited per function) plus the
 * reverse-mode ops tf.train.AdamOptimizer.minimize() derives from it
 * (multi_view_model/appearance_flow_model.py:77).
 *
 * Conventions
 *  - plain pointers + sizes, no torch/HIP types: a stream is passed as void* (hipStream_t).
 *  - every pointer is DEVICE memory owned by the caller; the library never allocates or
 *    frees device memory and keeps no global mutable state (except an optional recording plan,
 *    see mv3d_plan_*).  Scratch is passed in as (workspace, workspace_bytes).
 *  - all calls are asynchronous on `stream` and return 0 (MV3D_OK) or a negative MV3D_E_*;
 *    shape/alignment violations are rejected BEFORE anything is launched.
 *    mv3d_last_error() returns a thread-local message for the last failure.
 *  - activations are NHWC; a tensor may be a channel slice of a wider buffer: `*_ld` is the
 *    element stride between consecutive pixels (>= channels).  This makes tf.concat /
 *    tf.split on the channel axis free (main_model.py:94,131).
 *  - conv filters HWIO [kh,kw,Cin,Cout] (tf_utils.py:76), deconv filters [kh,kw,Cout,Cin]
 *    (tf_utils.py:94), fc matrices [in,out] (tf_utils.py:61).  Both filter kinds are
 *    [kh,kw,C_image_side,C_feature_side].
 *  - dtype: MV3D_F32 only in this round (IEEE fp32 in/out, fp32 MFMA accumulate).
 */
#ifndef MV3D_HIP_H
#define MV3D_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MV3D_OK = 0, MV3D_E_INVAL = -1, MV3D_E_HIP = -2, MV3D_E_WORKSPACE = -3, MV3D_E_UNSUPPORTED = -4 };
enum { MV3D_F32 = 0 };
/* activation kinds: value = f1*x + f2*|x| forms of tf_utils.py:25-33, tf.nn.tanh (main_model.py:79) */
enum { MV3D_ACT_NONE = 0, MV3D_ACT_LRELU = 1, MV3D_ACT_RELU = 2, MV3D_ACT_TANH = 3 };

/* Geometry of one conv2d / conv2d_transpose layer.  The IMAGE side is the strided-into tensor
 * (conv input, deconv output); the FEATURE side is the other one (conv output, deconv input):
 * Ho = ceil(H/sh), Wo = ceil(W/sw), TF 'SAME' padding (pad_before = total/2). */
typedef struct mv3d_conv_geom {
    int32_t N;              /* batch */
    int32_t H, W, C;        /* image side  */
    int32_t Ho, Wo, K;      /* feature side */
    int32_t kh, kw, sh, sw;
    int32_t img_ld, feat_ld;/* pixel strides (elements) of the image-/feature-side tensors */
    int32_t dtype;          /* MV3D_F32 */
} mv3d_conv_geom;

/* Fused epilogue applied to the tensor a kernel produces.
 *   y = act(acc + bias)                  (forward: tf_utils.py:82 '+ b', :25-33 activations)
 *   y = acc * act'(ref)                  (backward: the producing layer's activation gradient,
 *                                         evaluated from its saved OUTPUT `ref`; TF: sign(0)=0)
 * gmask_ref has the shape of the produced tensor, pixel stride gmask_ld. */
typedef struct mv3d_epilogue {
    const void* bias;       /* [channels] or NULL */
    int32_t act;            /* MV3D_ACT_* applied to the result */
    float leak;             /* lrelu leak (tf_utils.py:29: 0.2) */
    int32_t gmask_act;      /* MV3D_ACT_* whose derivative multiplies the result, or NONE */
    float gmask_leak;
    const void* gmask_ref;
    int32_t gmask_ld;
} mv3d_epilogue;

const char* mv3d_version(void);
const char* mv3d_last_error(void);
/* Diagnostics: replace the mask of disabled dispatch rungs (environment MV3D_DISABLE at load; bits in DESIGN.md 4.5);
 * returns the previous mask.  Results never change beyond rounding; 4096 selects the exact fp32-MFMA kernels. */
int mv3d_set_diagnostics(int mask);
/* Tuning: the number of CUs the following conv / deconv filter-gradient calls (and their workspace queries) spread their
 * partial-filter slabs over; 0 restores the default (MV3D_WG_CUS, 128 = half the chip: those launches normally share it with
 * the data-gradient chain).  Returns the previous value.  Results never change beyond summation order. */
int mv3d_set_wgrad_cus(int cus);

/* ---- input side (host): the reference's TFRecord shards, multi_view_model/utils/read_tf_records.py:46-85 -----------------
 * mv3d_tfrecord_read copies feature k of up to max_records records into dst[k] + (first + i) * sizes[k] (host memory, e.g. a
 * pinned batch buffer): kinds[k] = 0 a single bytes value of exactly sizes[k] bytes (raw uint8 image), 1 a float list of
 * sizes[k] / 4 values.  *nread < max_records only at the end of the file.  CRC-32C of every record is checked when the
 * reader was opened with verify_crc != 0.  mv3d_u8_to_unit_f32: device-side uint8 -> float32 / 255 (read_tf_records.py:111). */
typedef struct mv3d_tfrecord_reader mv3d_tfrecord_reader;
int mv3d_tfrecord_open(const char* path, int verify_crc, mv3d_tfrecord_reader** out);
int mv3d_tfrecord_read(mv3d_tfrecord_reader* r, int max_records, int first, int nfeat, const char* const* names, const int* kinds,
                       const size_t* sizes, void* const* dst, int* nread);
void mv3d_tfrecord_close(mv3d_tfrecord_reader* r);
int mv3d_u8_to_unit_f32(int64_t count, const void* src, void* dst, void* stream);

/* The reference's process_image (read_tf_records.py:88-112) for records whose size differs from the model's input, one launch:
 * src uint8 [n, hs, ws, c] -> central square crop of side S = min(hs, ws) (rows / columns from (side - S) / 2) -> TensorFlow 1.3
 * ResizeBicubic, align_corners = False, S x S -> ho x wo -> / 255 -> dst float32 [n, ho, wo, c]; no clipping.  Per axis, all in
 * fp32 without contraction: scale = (float)S / (float)out, loc = scale * (float)o, fl = floor(loc), off = lrintf((loc - fl) * 1024),
 * taps fl-1 .. fl+2 clamped to [0, S-1], weights from TF's coefficient table (A = -0.75) at off and 1024 - off; horizontal pass
 * first, then vertical, each ((v0*w0 + v1*w1) + v2*w2) + v3*w3 (input path).  S == out reproduces
 * mv3d_u8_to_unit_f32 bitwise.
 * MV3D_E_INVAL before any launch: a null pointer; n, hs, ws, ho, wo < 1; c outside 1 .. 4; a side above 4096; dst not 16-byte
 * aligned; n*hs*ws*c or n*ho*wo*c >= 2^31 - 2^21 (32-bit indices).  Allocates nothing, keeps no state. */
int mv3d_u8_process_image(const void* src, int n, int hs, int ws, int c, void* dst, int ho, int wo, void* stream);

/* ---- colour augmentation: ONE pointwise colour map per sample, applied in place to all of the sample's colour views -----------
 * The reference has no augmentation and TensorFlow was never run against this: the contract below is the project's own, and
 * augment.color_augment_host is its numpy twin and the authority (input path: colour augmentation).
 * images: a HOST array of `views` (1 .. 8) device pointers, each float32 [n, h, w, 3], 16-byte aligned, no two overlapping; read at
 * call time and handed to the kernels by value.  params: device float32 [n, 4] = brightness delta db, saturation factor fs, hue
 * delta dh, contrast factor fc of sample i.  stages: which stages run; a stage whose bit is clear is skipped, not run with a
 * neutral value.  Every operation is an fp32 operation that rounds on its own (no contraction), every division is correctly
 * rounded; clip(x) = x < 0 ? 0 : x > 1 ? 1 : x; max / min are a > b ? a : b / a < b ? a : b, left to right.  Per pixel (r, g, b):
 *   BRIGHTNESS  c = c + db
 *   SATURATION | HUE (one HSV round trip for both)
 *               c = clip(c); v = max(r, g, b); mn = min(r, g, b); range = v - mn; s = v > 0 ? range / v : 0; norm = 1 / (6 * range)
 *               h = r == v ? (g - b) * norm : g == v ? (b - r) * norm + 2.0f/6.0f : (r - g) * norm + 4.0f/6.0f
 *               h = range <= 0 ? 0 : h;  h = h < 0 ? h + 1 : h
 *               SATURATION: s = clip(s * fs)      HUE: h = h + dh      always: h = h - floor(h)
 *               c = s * v; m = v - c; d = h * 6; k = min((int)d, 5); f = d - 2 * floor(d / 2); x = c * (1 - |f - 1|)
 *               (r, g, b) = m + (c,x,0) (x,c,0) (0,c,x) (0,x,c) (x,0,c) (c,0,x) for k = 0 .. 5
 *   CONTRAST    c = (c - pivot[ch]) * fc + pivot[ch]
 *   always      c = clip(c)   (so a bicubic overshoot of the input is clipped whenever any stage runs)
 * The device evaluates clip, max and min with the hardware's clamp / max3 / min3 and the hue branch as one (a - b) * norm + offset
 * with the operands selected first: the same VALUES for every finite input (a zero may carry the other sign, which no later
 * operation turns into a different non-zero value); NaN inputs are outside the contract.
 * pivot[ch] of sample i: the mean of channel ch over ALL `views` images of the sample, of the input values, summed in double in a
 * fixed order, divided by views * h * w in double and rounded to float once.  The order: an image is cut into chunks of 4096 pixels;
 * thread t of 256 owns the pixel quads t + 256 k (k = 0 .. 3) of a chunk and adds their pixels in ascending order, one double per
 * channel; the pixels behind the last whole quad (h * w & 3 of them) belong to the thread that would own that quad; the 256 sums
 * are added as sum_common.h states (xor butterfly per wave, ((w0 + w1) + w2) + w3); the chunk sums are then added views ascending,
 * chunks ascending within a view.  Nothing depends on the grid or the device; no atomics, no global state.
 * Two launches with MV3D_AUG_CONTRAST (the chunk sums into `workspace`, 24 bytes per sample, view and chunk; then the map), one
 * without it, which leaves the workspace untouched.
 * MV3D_E_INVAL before any launch: images, params or workspace NULL, a NULL view; views outside 1 .. 8; n, h or w < 1; n*h*w*3 >=
 * 2^31 - 2^21 (32-bit indices); stages 0 or with unknown bits; a view or params not 16-byte aligned; two views
 * that are equal or overlap.  MV3D_E_WORKSPACE: workspace smaller than mv3d_color_augment_workspace_bytes() or not 16-byte aligned.
 * Kernel labels: color_augment_sums_kernel, color_augment_apply_kernel. */
enum { MV3D_AUG_BRIGHTNESS = 1, MV3D_AUG_SATURATION = 2, MV3D_AUG_HUE = 4, MV3D_AUG_CONTRAST = 8 };
size_t mv3d_color_augment_workspace_bytes(int n, int views, int h, int w);
int mv3d_color_augment(void* const* images, int views, int n, int h, int w, const void* params, unsigned stages,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- geometric augmentation: flip, centred zoom-in and window shift, ONE transform per sample for all of its views -------------
 * The three transforms that are exact for a pinhole camera on a turntable (input path: geometric augmentation): a
 * left-right mirror of every view (the scene reflected in the vertical plane through camera 0's axis: disp = (el1 - el0, az1 - az0)
 * becomes (el1 - el0, -(az1 - az0))), a longer focal length and a moved principal point (disp unchanged).  No in-plane rotation.
 * The reference has no augmentation and TensorFlow was never run against this: the contract is the project's own, and
 * augment.geom_augment_host is its numpy twin and the authority.
 * src, dst: HOST arrays of `views` (1 .. 16) device pointers, view v float32 [n, h, w, channels[v]] with channels[v] 1 or 3 (a HOST
 * array, too); read at call time and handed to the kernel by value.  Out of place: no destination equals or overlaps a source or
 * another destination.  params: device float32 [n, 4] = [m, inv, cxo, cyo] of sample i: m 0 or 1 (flip), inv = 1 / s of the zoom
 * s >= 1, cxo = cx + ox and cyo = cy + oy with cx = (w - 1) / 2, cy = (h - 1) / 2 and the window offsets ox, oy in source pixels,
 * each computed in double on the host and rounded once; finite.  disp: device float32 [n, 2], changed in place, or NULL.
 * Every operation is an fp32 operation that rounds on its own (no contraction).  For output pixel (x, y) of sample i:
 *   xp = m ? (w - 1) - x : x
 *   xs = (xp - cx) * inv + cxo;  xs = min(max(xs, 0), w - 1)
 *   ys = (y  - cy) * inv + cyo;  ys = min(max(ys, 0), h - 1)
 *   3 channels: x0 = floor(xs), x1 = min(x0 + 1, w - 1), fx = xs - x0; y0, y1, fy likewise; with a, b = src[y0][x0], src[y0][x1] and
 *               c, d = src[y1][x0], src[y1][x1]: top = a + (b - a) * fx; bot = c + (d - c) * fx; out = top + (bot - top) * fy
 *               per channel (this lerp returns a for fx = 0 and keeps a constant image constant to the bit)
 *   1 channel:  nearest: xi = min((int)floor(xs + 0.5f), w - 1), yi likewise; out = src[yi][xi].  Single-channel views are masks and
 *               depth maps: a mask stays in {0, 1} and depth is never blended across a silhouette.  Under zoom a colour edge and
 *               its mask edge may therefore differ by up to half a pixel, which is accepted.
 *   disp[i][1] = m ? -disp[i][1] : disp[i][1]   (disp[i][0] untouched)
 * The clamp keeps every read in bounds whatever the parameters hold.  One launch per call, no atomics, no workspace, no state;
 * the grid follows from the work alone and the result does not depend on it.
 * MV3D_E_INVAL before any launch: src, dst, channels or params NULL, a NULL view; views outside 1 .. 16; a channel count other
 * than 1 or 3; n, h or w < 1; n*h*w*3 >= 2^31 - 2^21 (32-bit indices); a view, params or a non-NULL disp not 16-byte aligned; any
 * two of the source and destination buffers equal or overlapping.  Kernel label: geom_augment_kernel. */
int mv3d_geom_augment(const void* const* src, void* const* dst, const int* channels, int views, int n, int h, int w,
                      const void* params, void* disp, void* stream);

/* CRC-32C of a host buffer: the record checksum of the reference's TFRecord shards (multi_view_model/utils/read_tf_records.py:46-48
 * reads them through tf.TFRecordReader); used by dynamic_multiview_3d_amd/read_tf_records.py */
uint32_t mv3d_crc32c(const void* data, size_t n);

/* ---- conv2d: tf.nn.conv2d(x, w, [1,sh,sw,1], 'SAME') + b  (tf_utils.py:81-82) ------------- */
/* y[N,Ho,Wo,K] = epi( x[N,H,W,C] (*) w[kh,kw,C,K] ) */
int mv3d_conv2d_fwd(const mv3d_conv_geom* g, const void* x, const void* w, void* y,
                    const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
/* dx[N,H,W,C] = epi( Conv2DBackpropInput(dy[N,Ho,Wo,K], w) ) */
int mv3d_conv2d_dgrad(const mv3d_conv_geom* g, const void* dy, const void* w, void* dx,
                      const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
/* dw[kh,kw,C,K] = Conv2DBackpropFilter(x, dy);  db[K] = BiasAddGrad(dy) (db may be NULL) */
int mv3d_conv2d_wgrad(const mv3d_conv_geom* g, const void* x, const void* dy, void* dw, void* db,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- conv2d_transpose: tf.nn.conv2d_transpose(x, w, output_shape, strides) (tf_utils.py:96-97)
 * x is the FEATURE side [N,Ho,Wo,K], y the IMAGE side [N,H,W,C], w [kh,kw,C,K]; no bias in the
 * reference (epi->bias must be NULL unless the caller wants one). */
int mv3d_deconv2d_fwd(const mv3d_conv_geom* g, const void* x, const void* w, void* y,
                      const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
int mv3d_deconv2d_dgrad(const mv3d_conv_geom* g, const void* dy, const void* w, void* dx,
                        const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
int mv3d_deconv2d_wgrad(const mv3d_conv_geom* g, const void* x, const void* dy, void* dw,
                        void* workspace, size_t workspace_bytes, void* stream);
/* bytes of scratch the six calls above may need for this geometry (max over them) */
size_t mv3d_conv_workspace_bytes(const mv3d_conv_geom* g);
/* the part of it the filter-gradient call of this geometry needs (its per-slab partial sums): what a caller that gives every
 * layer its own workspace (mv3d_grad_finalize_*) has to reserve per layer */
size_t mv3d_conv_wgrad_workspace_bytes(const mv3d_conv_geom* g);

/* ---- prepared filters (optional) -------------------------------------------------------------
 * The matrix-core convolution kernels read the filter split into bf16 hi/lo parts in MFMA fragment order.
 * By default each call converts its filter into the workspace (one extra small launch).  A caller that knows
 * its filters stay constant over several calls -- the reference's train step uses every filter in the forward
 * pass and again in the backward-data pass before tf.train.AdamOptimizer updates it (appearance_flow_model.py:77)
 * -- binds one caller-owned buffer per (filter, operation), commits the job table, and calls
 * mv3d_filter_cache_refresh() once after every weight update: ONE launch converts all bound filters and the
 * convolution calls that find their filter pointer in the cache skip their own conversion.
 * The cache is process-global (guarded by a mutex); the library never frees the bound buffers. */
enum { MV3D_FILTER_CONV_FWD = 0, MV3D_FILTER_CONV_DGRAD = 1, MV3D_FILTER_DECONV_FWD = 2, MV3D_FILTER_DECONV_DGRAD = 3 };
/* bytes of the prepared copy for this geometry / operation; 0 = the operation does not take one */
size_t mv3d_filter_prepared_bytes(const mv3d_conv_geom* g, int op);
int mv3d_filter_cache_bind(const mv3d_conv_geom* g, int op, const void* w, void* prepared, size_t prepared_bytes);
/* device bytes of the job table for the current bindings; commit uploads it (synchronises `stream`) */
size_t mv3d_filter_cache_table_bytes(void);
int mv3d_filter_cache_commit(void* table_dev, size_t table_bytes, void* stream);
/* one launch: convert every bound filter (recordable in a plan) */
int mv3d_filter_cache_refresh(void* stream);
int mv3d_filter_cache_clear(void);

/* ---- linear: tf.matmul(x, M) + b  (tf_utils.py:67) ------------------------------------------
 * x [B,in] (row stride x_ld), M [in,out] dense, y [B,out] (row stride y_ld). */
int mv3d_fc_fwd(int B, int in, int out, const void* x, int x_ld, const void* M, void* y, int y_ld,
                const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
int mv3d_fc_dgrad(int B, int in, int out, const void* dy, int dy_ld, const void* M, void* dx, int dx_ld,
                  const mv3d_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream);
int mv3d_fc_wgrad(int B, int in, int out, const void* x, int x_ld, const void* dy, int dy_ld,
                  void* dM, void* db, void* workspace, size_t workspace_bytes, void* stream);
/* Filter gradient AND data gradient of one small linear layer in ONE launch (both read dy; the angle MLP's a1 / a2,
 * appearance_flow_model.py:101-103): the results are those of mv3d_fc_wgrad followed by mv3d_fc_dgrad, bit for bit.  Layers
 * that are not "small" (the streaming fc kernels take them) are run as those two calls. */
int mv3d_fc_wgrad_dgrad(int B, int in, int out, const void* x, int x_ld, const void* dy, int dy_ld, const void* M,
                        void* dM, void* db, void* dx, int dx_ld, const mv3d_epilogue* dx_epi,
                        void* workspace, size_t workspace_bytes, void* stream);
/* A chain of 2..4 small linear layers (every width <= 64), y_l = act_l(y_{l-1} M_l + b_l), in ONE launch: a workgroup carries
 * four batch rows through all layers (activations stay in LDS, every y_l is also stored: the reverse pass needs it).  The
 * results are those of nlayers mv3d_fc_fwd calls, bit for bit. */
#define MV3D_FC_CHAIN_MAX 4
typedef struct mv3d_fc_chain_layer {
    const void* M;        /* [in, out], in = the previous layer's out (first layer: mv3d_fc_chain.in) */
    const void* bias;     /* [out] or NULL */
    void* y;              /* [B, out], row stride y_ld */
    int32_t y_ld, out;
    int32_t act;          /* MV3D_ACT_* */
    float leak;
} mv3d_fc_chain_layer;
typedef struct mv3d_fc_chain {
    int32_t B, nlayers, in, x_ld;
    const void* x;        /* [B, in], row stride x_ld */
    mv3d_fc_chain_layer l[MV3D_FC_CHAIN_MAX];
} mv3d_fc_chain;
int mv3d_fc_chain_fwd(const mv3d_fc_chain* chain, void* stream);
size_t mv3d_fc_workspace_bytes(int B, int in, int out);

/* ---- element-wise pieces -------------------------------------------------------------------- */
/* y = act(x) on [rows, ch] with row strides (standalone form of tf_utils.py:25-33 / tanh) */
int mv3d_act_fwd(int64_t rows, int ch, const void* x, int x_ld, void* y, int y_ld, int act, float leak, void* stream);
/* dx = dy * act'(ref) with ref = the activation's OUTPUT (sign(0) = 0) */
int mv3d_act_bwd(int64_t rows, int ch, const void* dy, int dy_ld, const void* ref, int ref_ld,
                 void* dx, int dx_ld, int act, float leak, void* stream);
/* strided copy / accumulate of [rows, ch] blocks (tf.concat/tf.split glue that cannot be a view,
 * tf.tile of the angle code over 4x4: multiobject_appflow.py:148-150):
 * dst[r*dst_ld + c] (+)= src[(r / src_row_div) * src_ld + c] */
int mv3d_copy2d(int64_t rows, int ch, const void* src, int64_t src_ld, int64_t src_row_div,
                void* dst, int64_t dst_ld, int accumulate, void* stream);
/* dst[g, c] = sum_{r < group} src[(g*group + r)*src_ld + c]   (gradient of the tile above) */
int mv3d_group_sum(int64_t groups, int group, int ch, const void* src, int64_t src_ld, void* dst, int64_t dst_ld, void* stream);

/* ---- warp + resampler: warp_pts_layer + resample_layer (tf_utils.py:35-52) ------------------
 * flow [N,H,W,2] (pixel stride flow_ld); warp = flow + coords where coords[...,0] = ROW index,
 * coords[...,1] = COLUMN index (tf_utils.py:48-51) and tf.contrib.resampler reads warp[...,0]
 * as x (column) and warp[...,1] as y (row); zero outside.
 * src [N,Hs,Ws,C] dense.  gen [N,H,W,C] dense.  warp_out (optional) [N,H,W,2] dense. */
int mv3d_warp_resample_fwd(int N, int H, int W, int Hs, int Ws, int C, const void* src, const void* flow, int flow_ld,
                           void* warp_out, void* gen, void* stream);
/* dflow[N,H,W,2] (pixel stride dflow_ld) = resampler grad w.r.t. warp (= grad w.r.t. flow) */
int mv3d_warp_resample_bwd(int N, int H, int W, int Hs, int Ws, int C, const void* src, const void* flow, int flow_ld,
                           const void* dgen, void* dflow, int dflow_ld, void* stream);
/* The appearance-flow head in one pass (appearance_flow_model.py:127-130 + tf_utils.py:18-23): gen = resample(src, flow +
 * coords); loss_accum[0] += weight * mean_{n,h,w} sum_c f(gen - target) (kind 2 squared, 1 absolute); dflow (optional) =
 * d(weight * loss)/dflow.  Same arithmetic as mv3d_warp_resample_fwd -> mv3d_pixel_loss -> mv3d_warp_resample_bwd with the
 * loss gradient kept on chip.  target [N,H,W,C] with pixel stride target_ld; C <= 4. */
int mv3d_warp_resample_loss(int N, int H, int W, int Hs, int Ws, int C, const void* src, const void* flow, int flow_ld,
                            const void* target, int target_ld, int kind, float weight, void* warp_out, void* gen,
                            void* dflow, int dflow_ld, void* loss_accum, void* stream);

/* ---- the plain resampler: tf.contrib.resampler.resampler(data, warp) for ANY warp (tf_utils.py:40-42) ----------
 * data [N,Hs,Ws,C] (pixel stride data_ld); warp [N,P,2] (pixel stride warp_ld), P = the product of the warp's middle
 * dimensions; warp[...,0] is x (column), warp[...,1] is y (row) -- NOT the transposed coords convention of the
 * mv3d_warp_resample_* entry points above.  out / dout [N,P,C] (pixel strides out_ld / dout_ld).
 *  - a point is valid iff x > -1 && y > -1 && x < Ws && y < Hs (NaN and +-inf are not); an invalid point gives out 0,
 *    dwarp 0, and adds nothing to ddata.
 *  - a tap outside the image reads 0 and its ddata contribution is dropped (never clamped onto a border pixel).
 *  - same fp32 expressions and operation order as mv3d_warp_resample_fwd / _bwd; dwarp sums the channels in order.
 * mv3d_resampler_bwd writes dwarp [N,P,2] and/or ddata [N,Hs,Ws,C] (either may be NULL, not both), overwriting them.
 * ddata is a scatter-add accumulated in 64-bit fixed point (scale 2^k with N*P*max|dout|*2^k <= 2^62): bitwise the same from
 * run to run; per element it is within (entries at that element) * N*P*max|dout|*2^-63 of the exact sum.  It needs
 * `workspace` (16-byte aligned) of mv3d_resampler_bwd_workspace_bytes() bytes; a call without ddata needs none.  dout must
 * be finite for ddata to be defined.
 * Limits (MV3D_E_UNSUPPORTED): Hs, Ws <= 2^24; N*P and N*Hs*Ws < 2^34; every operand with its stride < 2^40 floats;
 * N*Hs*Ws*C < 2^37. */
int mv3d_resampler_fwd(int N, int P, int Hs, int Ws, int C, const void* data, int data_ld,
                       const void* warp, int warp_ld, void* out, int out_ld, void* stream);
size_t mv3d_resampler_bwd_workspace_bytes(int N, int P, int Hs, int Ws, int C);
int mv3d_resampler_bwd(int N, int P, int Hs, int Ws, int C, const void* data, int data_ld,
                       const void* warp, int warp_ld, const void* dout, int dout_ld,
                       void* dwarp, int dwarp_ld, void* ddata, int ddata_ld,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- losses: euclidean_loss / l1_loss (tf_utils.py:18-23) -----------------------------------
 * loss_accum[0] += weight * mean_{n,h,w} sum_c f((a-b)*mask);  grad (optional, same shape as a,
 * dense) = d(weight*loss)/da.  kind 2 = squared (euclidean), 1 = absolute (l1); the third kind of loss term, SSIM, has its
 * own entry point (mv3d_ssim_loss below).  mask (optional)
 * is [pixels,1] and multiplies the difference (multiobject_appflow.py:239-242).
 * loss_accum must be zeroed by the caller before the first term (mv3d_fill). */
int mv3d_pixel_loss(int64_t pixels, int ch, const void* a, const void* b, const void* mask, int kind, float weight,
                    void* loss_accum, void* grad, void* stream);
/* same on channel-slice views (pixel strides *_ld), with the target read as b * b_scale and a per-pixel mask of stride
 * mask_ld: the mv3d losses slice a 4-channel prediction / target into colour and depth or mask parts
 * (mv3d/nobg_dm.py:85-92, mv3d/bg_nodm.py:85-93: gt_sm * 0.75, tf.multiply(.., sm)) */
int mv3d_pixel_loss_strided(int64_t pixels, int ch, const void* a, int a_ld, const void* b, int b_ld, float b_scale,
                            const void* mask, int mask_ld, int kind, float weight, void* loss_accum, void* grad, int grad_ld,
                            void* stream);
int mv3d_fill(void* dst, int64_t count, float value, void* stream);
/* The NEXT loss call of the calling thread (mv3d_pixel_loss*, mv3d_warp_resample_loss, mv3d_ssim_loss, mv3d_census_loss, mv3d_flow_smoothness, mv3d_flow_smoothness2, mv3d_multiscale_warp_loss, mv3d_flow_consistency, mv3d_warp_resample_occlusion_loss) stores its term into loss_accum instead of
 * adding it: the first term of a recorded step then needs no launch that clears the accumulator (tf.add_n over the terms of
 * appearance_flow_model.py:127-130 starts from the first one). */
int mv3d_loss_overwrite_next(void);

/* ---- image metrics: per-image L1, MSE and SSIM of a prediction against its target ---------------------------------
 * a, b [N,H,W,C] fp32 with pixel strides a_ld / b_ld (channel-slice views work), C in 1..4.  out [N,3] dense fp32:
 *   out[n][0] = mean over the H*W pixels of sum_c |a-b|     (the per-image form of l1_loss, tf_utils.py:22-23)
 *   out[n][1] = mean over the H*W*C elements of (a-b)^2     (PSNR = 10 log10(max_val^2 / out[n][1]) on the host)
 *   out[n][2] = SSIM (Wang et al. 2004) as tf.image.ssim computes it: F = the 11-tap Gaussian window (sigma 1.5, normalised to
 *               sum 1) applied separably over fully-inside windows only, so the map is (H-10) x (W-10) per channel;
 *               c1 = (0.01 max_val)^2, c2 = (0.03 max_val)^2, mx = F(a), my = F(b),
 *               lum = (2 mx my + c1) / (mx^2 + my^2 + c1),
 *               cs  = (2 F(a b) - 2 mx my + c2) / (F(a a + b b) - (mx^2 + my^2) + c2),
 *               value = mean of lum * cs over the windows and the C channels.
 * The window pass and the SSIM expression are fp32 without contraction (horizontal pass first, taps added in index order: the
 * map is the one metrics.py image_metrics_host computes in float32); the differences of L1 / MSE and every sum are in double.
 * a == b gives exactly {0, 0, 1}.  Sums run in a fixed order without atomics: the same inputs give the same bits, run after run.
 * The call allocates nothing and keeps no state outside `workspace` (16-byte aligned, mv3d_image_metrics_workspace_bytes()
 * bytes, which is 0 for a shape the entry refuses): the per-tile sums live there between its two launches.
 * MV3D_E_INVAL before any launch: N < 1; H or W < 11; C outside 1..4; H or W > 32768, or N * ceil(H/32) * ceil(W/32) >= 2^31
 * (the tile index is a 32-bit grid index; pixel offsets are 64-bit); a_ld or b_ld < C; max_val not finite or <= 0; a null
 * pointer; a, b or out not 4-byte aligned.  MV3D_E_WORKSPACE: workspace too small or not 16-byte aligned.  On any error out is
 * left untouched. */
size_t mv3d_image_metrics_workspace_bytes(int N, int H, int W, int C);
int mv3d_image_metrics(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, float max_val, void* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- SSIM as a training loss: value and gradient with respect to the prediction ---------------------------------------
 * a (prediction), b (target) [N,H,W,C] fp32 with pixel strides a_ld / b_ld (channel-slice views work), C in 1..4; Hv = H - 10,
 * Wv = W - 10.  With S = lum * cs the SSIM map of mv3d_image_metrics above (same window, c1, c2 and fp32 operation order):
 *   ssim_loss = 1 - (1 / (N*Hv*Wv*C)) * sum over images, windows and channels of S
 *             = 1 - the mean over the images of out[n][2] of mv3d_image_metrics;
 *   loss_accum[0] += weight * ssim_loss, or = weight * ssim_loss when mv3d_loss_overwrite_next() is pending on the calling thread
 *   (the flag is consumed; a recorded call keeps what it saw).  One thread adds, in stream order: no atomics.
 * grad (optional; NULL = value only) [N,H,W,C] with pixel stride grad_ld >= C receives d(weight * ssim_loss)/da: stored when
 * grad_accumulate == 0, added to what is there when grad_accumulate == 1 (a second differentiated term on one tensor).  Channels
 * outside the view are not touched.  Per window, with mx = F(a), my = F(b), sab = F(a b), s2 = F(a a + b b):
 *   A1 = 2 mx my + c1,  B1 = mx^2 + my^2 + c1,  A2 = 2 sab - 2 mx my + c2,  B2 = s2 - (mx^2 + my^2) + c2,  S = (A1/B1)(A2/B2)
 *   Dm = 2 (my (A2 - A1) - mx S (B2 - B1)) / (B1 B2)      Ds = 2 (A1/B1) / B2      Dq = -S / B2
 *   grad(q) = -weight / (N*Hv*Wv*C) * (Ft(Dm)(q) + b(q) Ft(Ds)(q) + 2 a(q) Ft(Dq)(q))
 * where Ft, the transpose of the valid window pass, is the same separable 11-tap filter over the Hv x Wv map zero-padded by
 * 10 on every side.  The window passes (horizontal first, taps added in index order, in both directions), S, the coefficients
 * and the combination are fp32 without contraction: the numbers metrics.py ssim_loss_host computes in float32.  The sum of S is
 * kept in double and reduced in a fixed order.  a == b gives a loss of exactly 0 and a gradient of exactly 0.
 * Every gradient element is written by exactly one thread; the same inputs give the same bits in value and gradient, run after
 * run and under plan replay; the value is the same bits with and without grad.  The call allocates nothing and keeps no state
 * outside `workspace` (16-byte aligned, mv3d_ssim_loss_workspace_bytes() bytes, which is 0 for a shape the entry refuses): the
 * per-tile sums live there between its two launches (plan labels ssim_loss_tile, ssim_loss_final).
 * MV3D_E_INVAL before any launch: N < 1; H or W < 11; C outside 1..4; H or W > 32768, or N * ceil(H/32) * ceil(W/32) >= 2^31;
 * a_ld or b_ld < C; grad given and grad_ld < C; grad_accumulate outside {0, 1}; max_val not finite or <= 0; weight not finite;
 * a, b, loss_accum or workspace null; a, b, loss_accum or grad not 4-byte aligned.  MV3D_E_WORKSPACE: workspace too small or not
 * 16-byte aligned.  On any error loss_accum and grad are left untouched and a pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_ssim_loss_workspace_bytes(int N, int H, int W, int C);
int mv3d_ssim_loss(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, float max_val, float weight,
                   void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace, size_t workspace_bytes,
                   void* stream);

/* The occlusion-masked form of mv3d_ssim_loss: the same arguments plus mask [N,H,W,1] fp32 with pixel stride mask_ld >= 1 (a
 * channel of a wider tensor works), indexed by the pixel of the prediction.  The mask is never differentiated and may hold any
 * finite values (mv3d_flow_occlusion_mask produces 0 / 1).  A window with origin (oy, ox) takes the mask at its centre, m_w =
 * m(oy + 5, ox + 5):
 *   ssim_loss_masked = M / count - Sm / count,   M = sum over c, w of m_w,   Sm = sum over c, w of fp32(m_w * S),
 *   count = N*Hv*Wv*C as in the unmasked entry (a masked window still counts: masked_euclidean_loss keeps its mean the same way);
 *   Dm, Ds, Dq of a window are each multiplied by m_w (one fp32 multiply) before the transposed passes.
 * M and Sm are double sums in the fixed order of the unmasked entry (plan labels ssim_loss_masked_tile, ssim_loss_masked_final; the
 * workspace holds 2 doubles per tile: mv3d_ssim_loss_masked_workspace_bytes(), 0 for a shape the entry refuses).  m == 1
 * everywhere gives the bits of mv3d_ssim_loss in the loss word and in every gradient element; m == 0 gives a term of +0 (for
 * weight >= 0) and a gradient of zeros; a == b gives exactly 0 under any mask; the term is linear in m.  Everything else (the
 * overwrite flag, grad_accumulate, determinism, value bits with and without grad) is as for mv3d_ssim_loss.
 * Errors: those of mv3d_ssim_loss, and MV3D_E_INVAL for mask_ld < 1, a null mask or a mask that is not 4-byte aligned, all before
 * any launch. */
size_t mv3d_ssim_loss_masked_workspace_bytes(int N, int H, int W, int C);
int mv3d_ssim_loss_masked(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask, int mask_ld,
                          float max_val, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- census (ternary) loss: value and gradient with respect to the prediction --------------------------------------------
 * The soft census transform of Meister et al. ("UnFlow") / Liu et al. ("DDFlow").  a (prediction), b (target) [N,H,W,C] fp32 with
 * pixel strides a_ld / b_ld (channel-slice views work), C in 1..4; radius r in {1, 2, 3}; K = (2r+1)^2 - 1 offsets o of the
 * (2r+1)^2 patch, centre excluded, row-major (dy outer, dx inner); Hv = H - 2r, Wv = W - 2r; a pixel is valid when its whole
 * patch is inside the image.
 *   g_x(p)   = (255 / max_val) (1/C) sum_c x(p,c)        intensity on the 0..255 scale: the constants mean what they mean in the
 *                                                        literature
 *   d_x(p,o) = g_x(p+o) - g_x(p)       R_x(p,o) = sqrt(0.81 + d_x^2)       t_x(p,o) = d_x / R_x
 *   u(p,o)   = t_a - t_b               e = u^2
 *   dist(p)  = (1/K) sum_o e / (0.1 + e)                 in [0, 1)
 *   root(p)  = sqrt(dist + eps^2)      rho(p) = dist / (root + eps)        the Charbonnier penalty root - eps, written so that
 *                                                                          dist == 0 gives exactly 0 whatever the rounding
 *   census_loss = (1 / (N Hv Wv)) sum over n and the valid p of rho(p)
 *   loss_accum[0] += weight * census_loss, or = weight * census_loss when mv3d_loss_overwrite_next() is pending on the calling
 *   thread (the flag is consumed; a recorded call keeps what it saw).  One thread adds, in stream order: no atomics.
 * grad (optional; NULL = value only) [N,H,W,C] with pixel stride grad_ld >= C receives d(weight * census_loss)/da: stored when
 * grad_accumulate == 0, one fp32 addition onto what is there when grad_accumulate == 1 (a second differentiated term on one
 * tensor).  Channels outside the view are never written.
 *   phi(p,o) = [0.1 / (0.1 + e)^2] 2 u 0.81 / R_a^3      rho'(p) = 1 / (2 root(p))
 *   dL/dg_a(q) = (1 / (K N Hv Wv)) ( sum_{o : q-o valid} rho'(q-o) phi(q-o, o) - [q valid] rho'(q) sum_o phi(q, o) )
 *   grad(q,c)  = weight (255 / (max_val C)) dL/dg_a(q)   the same for every channel c
 * Pixels outside the valid region still receive a gradient as neighbours.  a == b gives a loss of exactly 0 and a gradient of
 * exactly 0, because u == 0.
 * Every step is fp32 without contraction in the order metrics.py census_loss_host states (sqrt and division correctly rounded):
 * the numbers it computes in float32.  The tile sums of rho are kept in double and reduced in a fixed order.  Every gradient
 * element is written by exactly one thread; the same inputs give the same bits in value and gradient, run after run and under
 * plan replay; the value is the same bits with and without grad.  The call allocates nothing and keeps no state outside
 * `workspace` (16-byte aligned, mv3d_census_loss_workspace_bytes() bytes, which is 0 for a shape or radius the entry refuses):
 * the per-tile sums live there between its two launches (plan labels census_loss_tile, census_loss_final).
 * MV3D_E_INVAL before any launch: N < 1; radius outside 1..3; H or W < 2r+1; C outside 1..4; H or W > 32768, or
 * N * ceil(H/32) * ceil(W/32) >= 2^31; a_ld or b_ld < C; grad given and grad_ld < C; grad_accumulate outside {0, 1}; max_val or
 * eps not finite or <= 0; weight not finite; a, b, loss_accum or workspace null; a, b, loss_accum or grad not 4-byte aligned.
 * MV3D_E_WORKSPACE: workspace too small or not 16-byte aligned.  On any error loss_accum and grad are left untouched and a
 * pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_census_loss_workspace_bytes(int N, int H, int W, int C, int radius);
int mv3d_census_loss(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, int radius, float max_val,
                     float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The occlusion-masked form of mv3d_census_loss: the same arguments plus mask [N,H,W,1] fp32 with pixel stride mask_ld >= 1 (a
 * channel of a wider tensor works), indexed by the pixel of the prediction.  The mask is never differentiated, may hold any finite
 * values (mv3d_flow_occlusion_mask produces 0 / 1) and is read only at valid pixels.
 *   census_loss_masked = (1 / (N Hv Wv)) sum over n and the valid p of m(p) rho(p)
 * The count stays N Hv Wv (masked_euclidean_loss keeps its mean over all pixels the same way).  The product m(p) * rho(p) is formed
 * in fp32 and added into the double sum.  In the gradient rho'(p) becomes (0.5 / root(p)) * m(p), one fp32 multiply; everything
 * behind it is unchanged, so a masked pixel still receives a gradient as the neighbour of a visible one.  m == 1 everywhere gives
 * the bits of mv3d_census_loss in the loss word and in every gradient element; m == 0 gives a term of +0 (for weight >= 0) and a
 * gradient of zeros; a == b gives exactly 0 under any mask; the term is linear in m.  The workspace is that of
 * mv3d_census_loss_workspace_bytes(); the plan labels are census_loss_masked_tile, census_loss_masked_final.  Everything else (the
 * overwrite flag, grad_accumulate, determinism, value bits with and without grad) is as for mv3d_census_loss.
 * Errors: those of mv3d_census_loss, and MV3D_E_INVAL for mask_ld < 1, a null mask or a mask that is not 4-byte aligned, all
 * before any launch. */
int mv3d_census_loss_masked(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask, int mask_ld,
                            int radius, float max_val, float eps, float weight, void* loss_accum, void* grad, int grad_ld,
                            int grad_accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- edge-aware flow smoothness: value and gradient with respect to the flow --------------------------------------------
 * flow [N,H,W,2] fp32 with pixel stride flow_ld (a channel-slice view works), H, W >= 2; guide (optional; NULL with
 * guide_c == 0 = unguided) [N,H,W,guide_c] fp32 with pixel stride guide_ld, guide_c in 1..4.  With
 *   dx[n,i,j,c] = f[n,i,j+1,c] - f[n,i,j,c] (j < W-1),   dy[n,i,j,c] = f[n,i+1,j,c] - f[n,i,j,c] (i < H-1),
 *   wx[n,i,j] = exp(-(edge_alpha / guide_c) * sum_k |I[n,i,j+1,k] - I[n,i,j,k]|), wy the same along rows (both exactly 1 and
 *   edge_alpha ignored without a guide),   phi(d) = sqrt(d^2 + eps^2) - eps,   phi'(d) = d / sqrt(d^2 + eps^2):
 *   S = sum wx phi(dx) / (N H (W-1) 2) + sum wy phi(dy) / (N (H-1) W 2)
 *   loss_accum[0] += weight * S, or = weight * S when mv3d_loss_overwrite_next() is pending on the calling thread (the flag is
 *   consumed; a recorded call keeps what it saw; a call with loss_accum NULL leaves it pending).  One thread adds, in stream order.
 *   grad[n,i,j,c] (pixel stride grad_ld >= 2) = or += weight * ((wx phi'(dx))[i,j-1] - (wx phi'(dx))[i,j]) / Zx
 *                                                 + weight * ((wy phi'(dy))[i-1,j] - (wy phi'(dy))[i,j]) / Zy, out-of-range terms dropped:
 *   stored when grad_accumulate == 0, one fp32 addition onto what is there when grad_accumulate == 1 (the flow's gradient from
 *   its consumer).  The guide is not differentiated.  Channels outside the views are never written.
 * loss_accum and grad are each optional, not both NULL: value only, gradient only (one launch), or both in one pass.
 * Every step is fp32 without contraction in the order of metrics.py flow_smoothness_host at float32 (sqrt and division
 * correctly rounded; only exp may differ in the last place); the two sums behind S are kept in double and reduced in a fixed
 * order.  A constant flow gives a value of exactly 0 and a gradient of exactly 0.  Every gradient element has exactly one
 * writer; there are no atomics; the same inputs give the same bits, run after run and under plan replay, and the value's bits
 * do not depend on whether a gradient was asked for.  No state outside `workspace` (16-byte aligned,
 * mv3d_flow_smoothness_workspace_bytes() bytes, 0 for a shape the entry refuses): the per-tile sums live there between the two
 * launches (plan labels flow_smooth_tile, flow_smooth_final; the second only with loss_accum).
 * MV3D_E_INVAL before any launch: N < 1; H or W < 2; N * ceil(H/16) * ceil(W/64) >= 2^31 or an element index that overflows;
 * flow_ld < 2; guide_c outside 0..4, or non-zero with a NULL guide; guide_ld < guide_c; grad_ld < 2; grad_accumulate outside
 * {0, 1}; eps not finite or <= 0; edge_alpha not finite or < 0; weight not finite; flow NULL; loss_accum and grad both NULL;
 * workspace NULL; flow, guide, loss_accum or grad not 4-byte aligned.  MV3D_E_WORKSPACE: workspace too small or not 16-byte
 * aligned.  On any error loss_accum and grad are left untouched and a pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_flow_smoothness_workspace_bytes(int N, int H, int W);
int mv3d_flow_smoothness(int N, int H, int W, const void* flow, int flow_ld, const void* guide, int guide_c, int guide_ld,
                         float edge_alpha, float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- edge-aware SECOND-order flow smoothness: value and gradient with respect to the flow ----------------------------------
 * The operands, the argument list, the loss word (add by default, store after mv3d_loss_overwrite_next(), a call with loss_accum
 * NULL leaves the flag pending), grad_accumulate, the channel-slice strides, the workspace rules and the determinism are those of
 * mv3d_flow_smoothness; H, W >= 3.  Along an axis let c be the centre of a three-pixel stencil and -, + its neighbours (x centres
 * j = 1..W-2, y centres i = 1..H-2):
 *   d = (f[+] - f[c]) - (f[c] - f[-])                                     per flow channel
 *   s = sum_k (|I[c,k] - I[-,k]| + |I[+,k] - I[c,k]|), the two terms of a channel added in this order, channels in index order
 *   w = exp(-(edge_alpha / guide_c) * s): mathematically the product of mv3d_flow_smoothness's weights of the two edges the
 *       stencil spans; exactly 1, and no guide read, without a guide or with edge_alpha == 0
 *   S2 = sum w phi(dx) / (N H (W-2) 2) + sum w phi(dy) / (N (H-2) W 2),   phi, phi' as above
 *   grad[n,i,j,c] = or += weight * ((ex[i,j-1] - ex[i,j]) - (ex[i,j] - ex[i,j+1])) / Z2x
 *                          + weight * ((ey[i-1,j] - ey[i,j]) - (ey[i,j] - ey[i+1,j])) / Z2y,   e = w phi'(d), 0 where no stencil is centred
 * Every step is fp32 without contraction in the order of metrics.py flow_smoothness_host(order=2) at float32; the two sums behind
 * S2 are kept in double and reduced in a fixed order.  A flow whose first differences are exact and equal along each axis (a
 * constant flow, an affine flow with dyadic coefficients) gives a value of exactly 0 and a gradient of zeros under any guide.
 * Plan labels flow_smooth2_tile, flow_smooth2_final (the second only with loss_accum).
 * mv3d_flow_smoothness2_workspace_bytes() answers 0 for a shape the entry refuses (H or W < 3 among them).
 * Errors: those of mv3d_flow_smoothness with 3 in place of 2 as the smallest H, W; on any error loss_accum and grad are left
 * untouched and a pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_flow_smoothness2_workspace_bytes(int N, int H, int W);
int mv3d_flow_smoothness2(int N, int H, int W, const void* flow, int flow_ld, const void* guide, int guide_c, int guide_ld,
                          float edge_alpha, float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-scale photometric loss of a flow: value and gradient with respect to the full-resolution flow --------------------
 * src [N,Hs,Ws,C], target [N,H,W,C], flow [N,H,W,2], all fp32 with pixel strides src_ld / target_ld / flow_ld (channel-slice
 * views work); C in 1..4, levels L in 1..3, and H, W, Hs, Ws multiples of 2^L.  For level l = 1..L, f = 2^l:
 *   pool_l   halves level l-1 (level 0 = the input) in fp32: 0.25 * ((p00 + p01) + (p10 + p11)) of the 2 x 2 block
 *            p00 p01 / p10 p11 (row-major); it applies to src, to target and to both channels of the flow
 *   flow_l = pool_l(flow) * (1 / f)                          (exact)
 *   warp_l[n,I,J] = flow_l[n,I,J] + (I, J): channel 0 + the row index is what the sampler reads as x (column), channel 1 + the
 *            column index as y (row), the transposed convention of mv3d_warp_resample_fwd.  Pooling by f with aligned pixel
 *            centres maps a full-resolution coordinate x to (x - (f-1)/2) / f, so the coarse flow is exactly the block mean
 *   gen_l  = resample(pool_l(src), warp_l), zero outside: valid iff -1 < x < Ws/f and -1 < y < Hs/f, the fp32 expressions of
 *            mv3d_warp_resample_fwd / _bwd
 *   T_l    = mean over (n,I,J) of sum_c phi(gen_l - pool_l(target)); phi = the square (kind 2, the coarse euclidean_loss) or the
 *            absolute value (kind 1, the coarse l1_loss)
 *   term   = sum_l level_weights[l-1] * T_l    (level_weights: HOST array of `levels` floats, read at the call)
 *   loss_accum[0] += term, or = term when mv3d_loss_overwrite_next() is pending on the calling thread (the flag is consumed; a
 *   recorded call keeps what it saw; a call with loss_accum NULL leaves it pending).  One thread adds, in stream order.
 *   level_values (optional, device, `levels` floats; needs loss_accum) receives the unweighted T_l.
 *   grad[n,i,j,k] (pixel stride grad_ld >= 2) = or += sum_l level_weights[l-1] * G_l[n, i >> l, j >> l, k] / f^3 with
 *   G_l = d T_l / d warp_l the sampler's warp gradient (1 / f^2 from the block mean, 1 / f from the scaling): stored when
 *   grad_accumulate == 0; with grad_accumulate == 1 the levels are first added in level order in fp32 and the sum is added onto
 *   what is there with one fp32 addition.  src and target are not differentiated.  Channels outside the views are never written.
 * loss_accum and grad are each optional, not both NULL: value only, gradient only, or both in one call.
 * `workspace` (16-byte aligned, mv3d_multiscale_warp_loss_workspace_bytes() bytes, 0 for a shape the entry refuses) holds the
 * per-tile sums and the pyramids of src and target; the call keeps no other state.  pyramid_ready == 1 says the workspace
 * already holds the pyramids of these same src and target from an earlier call (the reverse-pass call of a step): the pooling
 * launch is skipped.  Launches (plan labels): multiscale_pyramid (unless pyramid_ready), multiscale_loss_tile,
 * multiscale_loss_final (only with loss_accum).
 * Every step is fp32 without contraction in the order of metrics.py multiscale_warp_loss_host at float32; the per-level sums
 * are kept in double, reduced in a fixed order, combined in level order in double and rounded once.  Every gradient element has
 * exactly one writer; there are no atomics; the same inputs give the same bits, run after run and under plan replay, and the
 * value's bits do not depend on whether a gradient was asked for.  gen_l == pool_l(target) at every level gives a value of
 * exactly 0 and a gradient of exactly 0.
 * MV3D_E_INVAL before any launch: N < 1; C outside 1..4; levels outside 1..3; H, W, Hs or Ws not a positive multiple of
 * 2^levels, or above 32768; 2^31 or more 32 x 32 tiles, or an element index that overflows; src_ld or target_ld < C; flow_ld or
 * grad_ld < 2; kind outside {1, 2}; grad_accumulate or pyramid_ready outside {0, 1}; src, flow, target or level_weights NULL; a
 * level weight that is not finite; loss_accum and grad both NULL; level_values without loss_accum; workspace NULL; src, flow,
 * target, loss_accum, level_values or grad not 4-byte aligned.  MV3D_E_WORKSPACE: workspace too small or not 16-byte aligned.
 * On any error loss_accum, level_values and grad are left untouched and a pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_multiscale_warp_loss_workspace_bytes(int N, int H, int W, int Hs, int Ws, int C, int levels);
int mv3d_multiscale_warp_loss(int N, int H, int W, int Hs, int Ws, int C, const void* src, int src_ld, const void* flow, int flow_ld,
                              const void* target, int target_ld, int levels, const float* level_weights, int kind, void* loss_accum,
                              void* level_values, void* grad, int grad_ld, int grad_accumulate, int pyramid_ready, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The masked form: mask [N,H,W,1] fp32 over the flow's grid with pixel stride mask_ld >= 1 (a channel of a wider tensor works);
 * it is not differentiated.  m_l = pool_l(mask), the pooling of the images and the flow, so a coarse pixel counts by its visible
 * share and a 0/1 mask pools exactly.
 *   T_l  = (1 / (N H_l W_l)) * sum over (n,I,J) of m_l(n,I,J) * sum_c phi(d_c): the count stays that of the unmasked term (as in
 *          mv3d_census_loss_masked and mv3d_ssim_loss_masked); a coarse pixel's channel sum s is formed in double as in the
 *          unmasked entry and the level sum adds (double)m_l * s
 *   dgen = (d_c * s_l) * m_l (kind 2) or (sign(d_c) * s_l) * m_l (kind 1): s_l unchanged, the mask multiplies last; G_l and grad
 *          follow from it as above
 * A mask of ones gives the value, level values and gradient of mv3d_multiscale_warp_loss bit for bit, a mask of zeros +0 and a
 * gradient of zeros, gen_l == pool_l(target) exactly 0 under any mask; value and gradient are linear in the mask.  The mask is
 * pooled inside the tile launch, beside the flow: the pyramid launch, the workspace (mv3d_multiscale_warp_loss_workspace_bytes(),
 * the same layout) and pyramid_ready mean what they mean above, and a pyramid_ready call reads the mask again.  Launches:
 * multiscale_pyramid (unless pyramid_ready), multiscale_loss_masked_tile, multiscale_loss_final (only with loss_accum).
 * Everything else, mv3d_loss_overwrite_next() included, is as above.  MV3D_E_INVAL in addition: mask_ld < 1; mask NULL or not
 * 4-byte aligned. */
int mv3d_multiscale_warp_loss_masked(int N, int H, int W, int Hs, int Ws, int C, const void* src, int src_ld, const void* flow, int flow_ld,
                                     const void* target, int target_ld, const void* mask, int mask_ld, int levels,
                                     const float* level_weights, int kind, void* loss_accum, void* level_values, void* grad, int grad_ld,
                                     int grad_accumulate, int pyramid_ready, void* workspace, size_t workspace_bytes, void* stream);

/* ---- forward-backward flow consistency over pair-swapped batches: value and gradient with respect to the flow --------------
 * flow [N,H,W,2] fp32 with pixel stride flow_ld (a channel-slice view works), N even, H == W >= 2.  The second half of the batch
 * holds the reversed pairs of the first (pair_swap.py): the partner of sample n is m = (n + N/2) mod N.  The sampler's convention
 * is the transposed one of mv3d_warp_resample_fwd: channel 0 + the ROW index is x (column), channel 1 + the COLUMN index is y
 * (row); it is why the images must be square and why the residual swaps the channels of the sample.  For pixel (i, j) of sample
 * n, f = flow[n,i,j,:]:
 *   x = f0 + i,  y = f1 + j;   valid iff 0 <= x <= W-1 and 0 <= y <= H-1 (NaN and inf are not): stricter than the sampler's
 *   -1 < x < W window, so that no tap with a non-zero weight lies outside the image (a flow does not fade to black)
 *   s = the bilinear sample of flow[m] at (row y, column x), both channels, with the sampler's tap and weight expressions; a tap
 *   at index W or H occurs only with weight 0, reads 0 and receives no gradient
 *   r0 = f0 + s1,  r1 = f1 + s0,  d = sqrt(r0^2 + r1^2 + eps^2),  phi = d - eps,  psi = (r0 / d, r1 / d)
 *   C = (sum over the valid pixels of phi) / (N H W),   valid_fraction = (valid pixels) / (N H W): the normaliser is fixed, an
 *   invalid pixel contributes 0 to the value and to every gradient
 *   loss_accum[0] += weight * C, or = weight * C when mv3d_loss_overwrite_next() is pending on the calling thread (the flag is
 *   consumed; a recorded call keeps what it saw; a call with loss_accum NULL leaves it pending).  One thread adds, in stream order.
 *   stats (optional, device, 2 floats; needs loss_accum) receives the unweighted C and valid_fraction.
 *   With k = weight / (N H W), grad (pixel stride grad_ld >= 2) receives
 *     gathered  at [n,i,j]: ((psi0 + gx) k, (psi1 + gy) k), with (gx, gy) what mv3d_warp_resample_bwd gives for data = flow[m]
 *               and dgen = (psi1, psi0); 0 for an invalid pixel
 *     scattered at every tap q of flow[m] with weight w_q: (w_q psi1, w_q psi0) summed over the pixels, the sum times k
 *   as grad = gathered + scattered (one fp32 addition): stored when grad_accumulate == 0, added onto what is there with one more
 *   fp32 addition when grad_accumulate == 1 (accumulate == contents + the stored gradient, bit for bit); one writer per element.
 *   The scatter is summed in 64-bit fixed point: llrint(w_q psi 2^K) is added with integer atomics into an int64 plane
 *   [N,H,W,2] in the workspace (cleared inside the call), K = 62 - ceil(log2(H W)) (48 at 128 x 128, never below 32).  An
 *   element receives at most one tap from each of the H W pixels of the partner sample and |w_q psi| < 1, so a sum stays within
 *   H W 2^K <= 2^62: overflow would need more than H W entries at one element, which cannot happen.  The tiled pass leaves the
 *   gathered part in a float2 plane of the workspace; a last pass converts the integer sum to fp32, multiplies by k, adds the
 *   gathered part and writes grad.  Error of the scattered
 *   part at an element: at most (entries at that element) * 2^-(K+1) * |k|, plus the one fp32 rounding of the conversion.
 * A non-finite value of flow[m] at a tap of a valid pixel makes that pixel's phi and psi NaN, as in the numpy twin: C and the
 * pixel's own gathered gradient are then NaN (the error stays visible), while its scattered entries, which the integer plane
 * cannot hold, are dropped (the twin drops them too).
 * loss_accum and grad are each optional, not both NULL.  Channels outside the views are never written.
 * Every step is fp32 without contraction in the order of metrics.py flow_consistency_host at float32 (sqrt and division
 * correctly rounded); only the sum behind C (double, fixed order), the valid count (integer-valued, exact) and the fixed-point
 * scatter differ from it.  Flows that invert each other on integer offsets, flow[n] = (a, b) and flow[m] = (-b, -a), give a value
 * of exactly 0 and gathered and scattered gradients of exactly 0 wherever the pixel is valid.  No floating-point atomics; the same
 * inputs give the same bits run after run, under plan replay, and for grad_accumulate 0 against 1 onto zeros; the value's bits
 * do not depend on whether a gradient was asked for.  No state outside `workspace` (16-byte aligned,
 * mv3d_flow_consistency_workspace_bytes() bytes, 0 for a shape the entry refuses): the int64 plane, the gathered plane and the per-tile sums.
 * Launches (plan labels): flow_consist_tile, flow_consist_scatter (only with grad), flow_consist_final.
 * MV3D_E_INVAL before any launch: N < 2 or odd; H != W; H < 2 or H > 32768; N * ceil(H/16) * ceil(W/64) >= 2^31 or an element
 * index that overflows; flow_ld < 2; grad_ld < 2; grad_accumulate outside {0, 1}; eps not finite, <= 0, or below 2^-63 (about
 * 1.1e-19: eps * eps must be a normal fp32 number, or its root is not eps again and the exact zeros are lost); weight not finite;
 * flow NULL; loss_accum and grad both NULL; stats without loss_accum; workspace NULL; flow, loss_accum, stats or grad not 4-byte
 * aligned.  MV3D_E_WORKSPACE: workspace too small or not 16-byte aligned.  On any error loss_accum, stats and grad are left
 * untouched and a pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_flow_consistency_workspace_bytes(int N, int H, int W);
int mv3d_flow_consistency(int N, int H, int W, const void* flow, int flow_ld, float eps, float weight, void* loss_accum, void* stats,
                          void* grad, int grad_ld, int grad_accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- occlusion masking of the appearance-flow head over pair-swapped batches ---------------------------------------------------
 * The conventions are those of mv3d_flow_consistency, restated: flow [N,H,W,2] fp32 with pixel stride flow_ld (a channel-slice view
 * works), N even, H == W >= 2; the second half of the batch holds the reversed pairs of the first (pair_swap.py), the partner of
 * sample n is m = (n + N/2) mod N; channel 0 + the ROW index is x (column), channel 1 + the COLUMN index is y (row).  For pixel
 * (i, j) of sample n, f = flow[n,i,j,:]:
 *   x = f0 + i,  y = f1 + j;   inside iff 0 <= x <= W-1 and 0 <= y <= H-1 (NaN and inf are not): the consistency term's strict
 *   window, not the sampler's
 *   s = the bilinear sample of flow[m] at (row y, column x), both channels, with the sampler's taps ff cc fc cf, its weights
 *   w = (dx dy, (1-dx)(1-dy), dx (1-dy), (1-dx) dy) and the order ((w0 ff + w1 cc) + w2 fc) + w3 cf; a tap at index W or H occurs
 *   only with weight 0 and reads 0
 *   r0 = f0 + s1,  r1 = f1 + s0,  lhs = r0 r0 + r1 r1,  rhs = alpha1 ((f0 f0 + f1 f1) + (s0 s0 + s1 s1)) + alpha2
 *   visible iff inside and lhs < rhs (a NaN on either side makes the comparison false: the pixel counts as occluded)
 *   mask[n,i,j] = 1.0f where visible, 0.0f where inside and not visible, and outside_visible ? 1.0f : 0.0f where not inside (the
 *   check cannot be made there: 1 keeps the plain loss on such pixels, 0 is UnFlow's choice)
 * Every step is fp32 without contraction in the order of metrics.py flow_occlusion_mask_host at float32.  The mask has no
 * gradient: it is a constant of the step.
 *
 * mv3d_flow_occlusion_mask: mask_out (optional) is [N,H,W] fp32 with pixel stride mask_ld >= 1 (a channel of a wider tensor
 * works; the other channels are never written).  stats (optional, device, 3 floats) receives the visible, occluded and outside
 * shares of N H W: integer counts, exact, added in a fixed order, the same bits on every run.  mask_out and stats are not both
 * NULL.  Only a call with stats needs the workspace (16-byte aligned, mv3d_flow_occlusion_mask_workspace_bytes() bytes, 0 for a
 * shape the entry refuses): it holds the per-tile counts.  Launches (plan labels): occl_mask, and occl_mask_stats behind it when
 * stats is given.
 * MV3D_E_INVAL before any launch: N < 2 or odd; H != W; H < 2 or H > 32768; N * ceil(H/32)^2 >= 2^31 or an element index that
 * overflows; flow_ld < 2; mask_ld < 1; alpha1 not finite or < 0; alpha2 not finite or <= 0; outside_visible outside {0, 1}; flow
 * NULL; mask_out and stats both NULL; an operand not 4-byte aligned; with stats: workspace NULL.  MV3D_E_WORKSPACE: workspace too
 * small or not 16-byte aligned.  On any error mask_out and stats are left untouched.
 *
 * mv3d_warp_resample_occlusion_loss: the occlusion-aware head in one tiled pass.  The arguments of mv3d_warp_resample_loss plus
 * alpha1, alpha2, outside_visible, an optional mask_out / mask_ld, optional stats and a workspace
 * (mv3d_warp_resample_occlusion_loss_workspace_bytes(), always needed).  Requires Hs == H == W == Ws, N even, C <= 4.  Produces
 *   gen (written unmasked) and warp_out (optional) with the bits of mv3d_warp_resample_fwd
 *   the mask above (the partner-flow taps sit at the same (row y, column x) as the image taps), into mask_out when given
 *   loss_accum[0] += weight * mean_{n,h,w} sum_c f((gen - target) * mask), f squared for kind 2 and absolute for kind 1 (the
 *   expressions of mv3d_pixel_loss_strided with a mask); = instead of += when mv3d_loss_overwrite_next() is pending on the calling
 *   thread (the flag is consumed; a recorded call keeps what it saw).  The fp32 terms are added in double per tile in a fixed
 *   order, the tiles in index order by a last launch: no floating-point atomics, the same bits on every run
 *   dflow (optional, pixel stride dflow_ld >= 2) = d(weight * loss) / dflow with the mask held constant: bit for bit what
 *   mv3d_flow_occlusion_mask, mv3d_warp_resample_fwd, mv3d_pixel_loss_strided(mask) and mv3d_warp_resample_bwd give in a row
 *   stats (optional, 3 floats) as above.
 * Launches (plan labels): occl_head_tile, occl_head_final.
 * MV3D_E_INVAL before any launch: the shape errors above; Hs != H or Ws != W; C outside 1..4; flow_ld < 2; target_ld < C; dflow
 * with dflow_ld < 2; mask_out with mask_ld < 1; kind outside {1, 2}; weight not finite; the alpha and outside_visible errors
 * above; src, flow, target, gen or loss_accum NULL; workspace NULL; an operand not 4-byte aligned.  MV3D_E_WORKSPACE: workspace
 * too small or not 16-byte aligned.  On any error loss_accum, stats, mask_out, gen, warp_out and dflow are left untouched and a
 * pending mv3d_loss_overwrite_next() stays pending. */
size_t mv3d_flow_occlusion_mask_workspace_bytes(int N, int H, int W);
int mv3d_flow_occlusion_mask(int N, int H, int W, const void* flow, int flow_ld, float alpha1, float alpha2, int outside_visible,
                             void* mask_out, int mask_ld, void* stats, void* workspace, size_t workspace_bytes, void* stream);
size_t mv3d_warp_resample_occlusion_loss_workspace_bytes(int N, int H, int W);
int mv3d_warp_resample_occlusion_loss(int N, int H, int W, int Hs, int Ws, int C, const void* src, const void* flow, int flow_ld,
                                      const void* target, int target_ld, int kind, float weight, float alpha1, float alpha2,
                                      int outside_visible, void* warp_out, void* gen, void* dflow, int dflow_ld, void* mask_out,
                                      int mask_ld, void* loss_accum, void* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Adam: tf.train.AdamOptimizer ApplyAdam (appearance_flow_model.py:77) -------
 *   alpha = lr*sqrt(1-beta2_power)/(1-beta1_power);  m += (g-m)(1-b1);  v += (g*g-v)(1-b2);
 *   p -= m*alpha/(sqrt(v)+eps).   One fused pass over a flat fp32 buffer; grad_scale multiplies g
 *   first (1/world_size after a SUM all-reduce). */
int mv3d_adam_step(int64_t count, void* p, const void* g, void* m, void* v, float lr, float beta1, float beta2,
                   float eps, float beta1_power, float beta2_power, float grad_scale, void* stream);

/* Device-resident optimiser state, so that a RECORDED step replays with the current bias correction:
 * state[MV3D_ADAM_LR .. MV3D_ADAM_GSCALE] floats (8 allocated).  mv3d_adam_step_dev is mv3d_adam_step with the scalars read
 * from it, and leaves up to 8 index ranges [skip_lo, skip_hi) (multiples of 4) untouched; mv3d_adam_advance multiplies the two
 * beta powers by their betas (tf.train.AdamOptimizer._finish, appearance_flow_model.py:77), one launch per step. */
enum { MV3D_ADAM_LR = 0, MV3D_ADAM_BETA1 = 1, MV3D_ADAM_BETA2 = 2, MV3D_ADAM_EPS = 3, MV3D_ADAM_BETA1_POWER = 4, MV3D_ADAM_BETA2_POWER = 5,
       MV3D_ADAM_GSCALE = 6, MV3D_ADAM_STATE_FLOATS = 8 };
int mv3d_adam_step_dev(int64_t count, void* p, const void* g, void* m, void* v, const void* adam_state, int nskip,
                       const int64_t* skip_lo, const int64_t* skip_hi, void* stream);
int mv3d_adam_advance(void* adam_state, void* stream);
/* linear_msra's filter gradient with the ApplyAdam update of that matrix fused into the epilogue (tf_utils.py:54-67 +
 * appearance_flow_model.py:77): M, adam_m, adam_v [in,out] are updated in place from dM = x^T dy, which never goes to memory
 * (24 instead of 32 B of HBM traffic per parameter over the two passes it replaces); db[out] (optional) receives the bias
 * gradient as mv3d_fc_wgrad writes it.  Single-GPU steps only: the data-parallel step needs the gradient itself.  The caller
 * orders this call behind the last reader of M (the layer's own data gradient).  _supported: 1 when the layer is one the fused
 * kernel takes, 0 when mv3d_fc_wgrad + mv3d_adam_step_dev must be used. */
int mv3d_fc_wgrad_adam(int B, int in, int out, const void* x, int x_ld, const void* dy, int dy_ld, void* M, void* adam_m, void* adam_v,
                       void* db, const void* adam_state, void* stream);
int mv3d_fc_wgrad_adam_supported(int B, int in, int out, int x_ld, int dy_ld);

/* ---- GD / Momentum: tf.train.GradientDescentOptimizer (ApplyGradientDescent) and tf.train.MomentumOptimizer (ApplyMomentum) ----
 * g *= grad_scale first, then in TF's order (fp32, no contraction):
 *   accum == NULL:  p -= g*lr                                          (momentum must be 0 and use_nesterov 0)
 *   accum != NULL:  a = a*mu + g;  p -= a*lr   |   p -= g*lr + (a*mu)*lr  (use_nesterov)
 * 12 (GD) / 20 (Momentum) B per parameter.  Neither optimiser has a per-step "advance". */
int mv3d_sgd_step(int64_t count, void* p, const void* g, void* accum, float lr, float momentum, int use_nesterov,
                  float grad_scale, void* stream);
/* Device state of the same 8-float record size and GSCALE index as the Adam state (nesterov: 0.0f or 1.0f); _dev reads the scalars
 * from it and leaves up to 8 index ranges untouched, as mv3d_adam_step_dev. */
enum { MV3D_SGD_LR = 0, MV3D_SGD_MOMENTUM = 1, MV3D_SGD_NESTEROV = 2, MV3D_SGD_GSCALE = 6, MV3D_SGD_STATE_FLOATS = 8 };
int mv3d_sgd_step_dev(int64_t count, void* p, const void* g, void* accum, const void* sgd_state, int nskip,
                      const int64_t* skip_lo, const int64_t* skip_hi, void* stream);
/* mv3d_fc_wgrad_adam with the Momentum (accum != NULL) or GD (accum == NULL) update of M fused into the epilogue (16 / 8 B of HBM
 * traffic per parameter); the layer set is mv3d_fc_wgrad_adam_supported's. */
int mv3d_fc_wgrad_sgd(int B, int in, int out, const void* x, int x_ld, const void* dy, int dy_ld, void* M, void* accum,
                      void* db, const void* sgd_state, void* stream);

/* ---- EMA weights: tf.train.ExponentialMovingAverage (moving_averages.assign_moving_average, zero_debias=False) -------------
 * Per element, fp32, in TF's order and without contraction (bit-exact against numpy):
 *   d = s - p;  u = d * one_minus_decay;  s = s - u
 * over `count` >= 1 floats (a scalar tail takes count & 3).  params is only read.  one_minus_decay is float32(1 - decay_t),
 * rounded once by the caller, and must lie in [0, 1].  Both pointers 16-byte aligned.  12 B of HBM traffic per parameter
 * (two loads, one store: the traffic of mv3d_sgd_step without a slot).  Kernel label: ema_kernel. */
int mv3d_ema_step(int64_t count, void* shadow, const void* params, float one_minus_decay, void* stream);
/* Exchanges two disjoint buffers of `count` >= 1 floats in place, bit for bit (NaN payloads included): the averaged weights
 * take the place of the weights without a third buffer.  Both pointers 16-byte aligned; a == b or an overlap is refused.
 * Kernel label: swap_kernel. */
int mv3d_swap_f32(int64_t count, void* a, void* b, void* stream);

/* ---- scheduled learning rate: state[MV3D_ADAM_LR] (= state[MV3D_SGD_LR], float 0 of an 8-float optimiser record) = lr --------
 * One workgroup, one plain store; the other 7 floats of the record are not touched.  The caller issues it with the rate of the
 * NEXT update, behind the last launch of this update that reads the record and ON THAT LAUNCH'S STREAM: a write in front of a
 * step could race the previous update's launches still in flight.  MV3D_E_INVAL: state NULL or not 4-byte aligned; lr negative,
 * NaN or infinite.  Kernel label: opt_set_lr_kernel. */
int mv3d_opt_set_lr(void* state, float lr, void* stream);

/* ---- decoupled weight decay (the decay of torch.optim.AdamW, behind the optimiser's update), alone or with the EMA fused -------
 * Over [lo, hi) intersected with a table of index ranges of the flat parameter buffer, per element, fp32, without contraction
 * (bit-exact against numpy, graph.weight_decay_rule):
 *   t = p * f;  p = p - t          f = float32(double(lr) * weight_decay), rounded once by the caller, in [0, 1)
 * An element whose t is 0 (p = +-0, f = 0, an underflowing product) keeps its bits: that differs from the two operations only
 * for p = -0, whose sign stays.
 * params / shadow: the BASES of the flat buffers, 16-byte aligned; lo, hi, and the table's bounds are absolute element indices.
 * ranges: DEVICE memory, nranges <= MV3D_DECAY_MAX_RANGES pairs of int64 [begin, end), sorted, disjoint, every bound a multiple
 * of 4 (the caller guarantees it: the table is not read on the host); ranges may reach outside [lo, hi).  lo is a multiple of 4;
 * hi is one too, or, in the fused form only, the unaligned end of the buffers (a scalar tail takes (hi - lo) & 3).  (The pure form
 * refuses an unaligned hi: every range bound is a multiple of 4 and the entry cannot know where the buffer ends, so it cannot tell
 * the buffer's end from a mistake; the feature's specification allowed the unaligned end in both forms -- a deliberate
 * departure.  The graph's flat buffers are padded to multiples of 64 floats, so no caller of the project meets it.)
 *   shadow == NULL  pure decay: a chunk (4096 floats) that meets no range is skipped without a load, elements outside the
 *                   ranges are neither read nor written; 8 B of HBM traffic per decayed element.  one_minus_decay is ignored.
 *   shadow != NULL  the EMA fused behind the decay: for EVERY element of [lo, hi)  d = s - p';  u = d * one_minus_decay;
 *                   s = s - u  (mv3d_ema_step's three operations in its order), p' the decayed value inside the ranges and p
 *                   outside them; 16 B per decayed element, 12 B elsewhere (the two separate launches move 8 + 12).
 * MV3D_E_INVAL before any launch: params NULL; a misaligned buffer or table; lo < 0, hi <= lo, lo & 3, hi & 3 without a shadow;
 * nranges outside 0 .. MV3D_DECAY_MAX_RANGES, or > 0 with ranges NULL; f outside [0, 1) or NaN; with a shadow one_minus_decay
 * outside [0, 1] or NaN.  Kernel labels: weight_decay_kernel, weight_decay_kernel<fused>. */
enum { MV3D_DECAY_MAX_RANGES = 1024 };
int mv3d_weight_decay_step(void* params, void* shadow /* NULL: no EMA */, int64_t lo, int64_t hi, const void* ranges, int nranges,
                           float f, float one_minus_decay, void* stream);

/* ---- global-norm gradient clipping (the tf.clip_by_global_norm step of a TF-1.x trainer, over ONE flat gradient buffer) ------
 * n = ||g||_2 * pre_scale over `count` >= 1 floats; s = clip_norm / n where n > clip_norm, else 1; out[0] = n, out[1] = s, and
 * slot 6 (MV3D_ADAM_GSCALE / MV3D_SGD_GSCALE) of each optimiser record given becomes pre_scale * s: the optimiser launch that
 * follows on the same stream multiplies every gradient by it, so no gradient is rewritten.  g is only read and 16-byte aligned;
 * out is 4-byte aligned (2 floats); state_a / state_b may each be NULL.  pre_scale (the 1 / world size of a data-parallel step)
 * is finite and > 0; clip_norm is > 0, +INFINITY = measure only (s is then always 1).  The workspace is the caller's, at least
 * mv3d_grad_clip_workspace_bytes(count) bytes (0 for count < 1; >= 8 * ceil(count / 16384)), 16-byte aligned: no global device
 * state, no atomics.  MV3D_E_INVAL before any launch: count < 1; g, out or workspace NULL; g not 16-byte, out / state_a / state_b
 * not 4-byte aligned; pre_scale or clip_norm out of range (NaN included).  MV3D_E_WORKSPACE: workspace too small or misaligned.
 *
 * Two launches.  grad_sumsq_kernel: a 4 B/element read stream; the buffer is cut into chunks of 16384 floats (256 threads x 16
 * float4; fixed, whatever the device and the grid), a workgroup walks chunks with a grid stride and writes ONE double per chunk.
 * grad_clip_final_kernel: one workgroup of 256 sums the chunk partials, thread 0 finishes.
 *
 * Order contract (the numpy twin graph.grad_clip_rule follows it; results are the same bits on every run and every grid):
 *   - every element is converted to double and squared: exact, 24 x 24 bits fit in 53
 *   - thread t of a chunk owns float4s t + 256 k, k = 0 .. 15, of that chunk and adds their squares to ONE double accumulator
 *     that starts at 0, in the order k = 0 .. 15, components x, y, z, w; elements at or past `count` (the partial last chunk,
 *     the count & 3 tail) count as 0
 *   - the 256 accumulators: xor butterfly with offsets 32, 16 .. 1 inside each wave of 64, then ((w0 + w1) + w2) + w3
 *   - final kernel: thread t adds the chunk sums t, t + 256, .. in index order to one double that starts at 0, then the same
 *     workgroup sum gives S
 *   - thread 0, fp32 and uncontracted but for the root: n = (float)sqrt(S) * pre_scale (sqrt in double, correctly rounded);
 *     s = n > clip_norm ? clip_norm / n : 1.0f; state[6] = pre_scale * s
 * Deliberate differences from tf.clip_by_global_norm:
 *   - not TF's clip * min(1 / n, 1 / clip): a step that is not clipped multiplies by exactly pre_scale and so keeps the bits of
 *     an unclipped step
 *   - a NaN norm compares false: the scale stays 1, the NaNs stay visible in the loss and in out[0] (TF would spread them)
 *   - an infinite norm gives scale 0 (the step is dropped)
 *   - the sums are double: a gradient with entries of 1e30 has a finite norm where an fp32 sum of squares overflows
 * Kernel labels: grad_sumsq_kernel, grad_clip_final_kernel. */
size_t mv3d_grad_clip_workspace_bytes(int64_t count);
int mv3d_grad_clip_scale(int64_t count, const void* g, float pre_scale, float clip_norm, void* out, void* state_a, void* state_b,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Pass 2 of mv3d_grad_clip_scale on its own: the grad_clip_final_kernel launch over chunk partials that are already in `workspace`
 * (written by mv3d_grad_clip_scale's first launch or by mv3d_grad_accumulate in MV3D_ACCUM_FINISH mode with sumsq_part; the
 * workspace is only read).  Same results, same order, same checks as mv3d_grad_clip_scale, g apart.  Kernel label:
 * grad_clip_final_kernel. */
int mv3d_grad_clip_finish(int64_t count, float pre_scale, float clip_norm, void* out, void* state_a, void* state_b,
                          const void* workspace, size_t workspace_bytes, void* stream);

/* ---- gradient accumulation: N micro-batches' gradients summed over ONE flat gradient buffer, one optimiser update behind them ---
 * `sum` and `g` hold `count` >= 1 floats each, are 16-byte aligned and do not overlap.  One launch per micro-batch, on the stream
 * of the reverse pass that wrote g:
 *   MV3D_ACCUM_STORE   sum[i] = g[i]             the first micro-batch: sum is not read and needs no memset; 8 B/element
 *   MV3D_ACCUM_ADD     sum[i] = sum[i] + g[i]    12 B/element
 *   MV3D_ACCUM_FINISH  g[i]   = sum[i] + g[i]    the last micro-batch, written into G: sum is only read; 12 B/element
 * STORE and ADD leave g as it is.  Because FINISH writes into g, the norm and every optimiser kernel behind it read the flat
 * gradient buffer as ever; the 1 / N of the mean goes into the gradient-scale slot of the optimiser records (slot 6), which
 * mv3d_grad_clip_scale / mv3d_grad_clip_finish write through their pre_scale.  The sum is ((g1 + g2) + g3) .., one fp32 addition
 * per element and launch, uncontracted; one writer per element, no atomics, no global device state: the same bits on every run
 * and every grid.  graph.grad_accum_rule is the numpy twin.
 *
 * The loss rides along: `loss` and `loss_sum` are one float each (4-byte aligned), both given or both NULL.  STORE: loss_sum =
 * loss; ADD: loss_sum = loss_sum + loss; FINISH: loss_sum = (loss_sum + loss) * loss_scale (the mean for loss_scale = 1 / N;
 * loss_scale is read by FINISH only).  One thread of the launch does it.
 *
 * sumsq_part != NULL (FINISH only; at least mv3d_grad_clip_workspace_bytes(count) bytes, 16-byte aligned): the launch also writes
 * one double per chunk of 16384 floats, the sum of squares of the values it STORED into g, by the order contract of
 * grad_sumsq_kernel above -- the same chunking, thread t owns float4s t + 256 k and adds their squares to one double in the
 * order k = 0 .. 15, x, y, z, w, elements at or past `count` count as 0, then the workgroup sum.  mv3d_grad_clip_finish on that
 * workspace then gives the bits mv3d_grad_clip_scale gives on the stored buffer, and the norm's 4 B/element read pass is saved.
 * (The loads of a chunk are issued in two rounds of 8 float4s per lane and buffer; the order of the additions does not depend
 * on it.)
 * MV3D_E_INVAL before any launch: count < 1; sum or g NULL, not 16-byte aligned, or overlapping; an unknown mode; one of loss /
 * loss_sum without the other, or not 4-byte aligned; sumsq_part outside FINISH.  MV3D_E_WORKSPACE: sumsq_part too small or
 * misaligned.
 * Kernel labels: grad_accum_store_kernel, grad_accum_add_kernel, grad_accum_finish_kernel, grad_accum_finish_sumsq_kernel. */
enum { MV3D_ACCUM_STORE = 0, MV3D_ACCUM_ADD = 1, MV3D_ACCUM_FINISH = 2 };
int mv3d_grad_accumulate(int64_t count, void* sum, void* g, int mode, const void* loss, void* loss_sum, float loss_scale,
                         void* sumsq_part, size_t sumsq_bytes, void* stream);

/* ---- gradient finalisation: the slab reductions of ALL filter gradients (+ their optimiser update) in one launch ------------
 * Replaces, on the recorded single-GPU step, the per-layer partial-filter reductions behind tf.gradients' Conv2DBackpropFilter
 * ops and the tf.train.AdamOptimizer ApplyAdam ops of every variable that is not an fc matrix (appearance_flow_model.py:77).
 * Between mv3d_grad_finalize_begin() and _commit() on this thread the filter-gradient entry points (mv3d_conv2d_wgrad,
 * mv3d_deconv2d_wgrad) leave their per-slab partial sums in the workspace they were given -- which the caller must then keep
 * untouched until the committed launch has run, i.e. one workspace per layer -- and record a segment instead of launching a
 * reduction.  mv3d_grad_finalize_add names a gradient range that is already final (fc biases, tiny fc layers) so that the
 * optimiser covers it too.  _table_bytes: device bytes the segment table needs for what has been collected so far.
 * _commit closes the collection, uploads the table (synchronously, at call / record time) and dispatches ONE launch that sums
 * every segment's slabs in the fixed order of the per-layer reduction (same bits) and
 *   adam_state == NULL: stores the gradients where the wgrad calls were told to (grads/params/adam_m/adam_v ignored);
 *   adam_state != NULL: applies ApplyAdam to each element instead (mv3d_adam_step_dev's arithmetic, same bits); every
 *                       segment must lie inside the flat buffer `grads`, whose layout params / adam_m / adam_v share.
 * _abort drops an open collection.  (table may be NULL only while recording a plan without a device, which can never run.) */
int mv3d_grad_finalize_begin(void);
int mv3d_grad_finalize_add(void* grad, int64_t count);
size_t mv3d_grad_finalize_table_bytes(void);
int mv3d_grad_finalize_commit(void* table, size_t table_bytes, void* grads, void* params, void* adam_m, void* adam_v,
                              const void* adam_state, void* stream);
/* _commit with ApplyMomentum (accum != NULL) or ApplyGradientDescent (accum == NULL) in place of ApplyAdam (mv3d_sgd_step_dev's
 * arithmetic, same bits); sgd_state is required (gradients only: mv3d_grad_finalize_commit with adam_state NULL). */
int mv3d_grad_finalize_commit_sgd(void* table, size_t table_bytes, void* grads, void* params, void* accum, const void* sgd_state,
                                  void* stream);
int mv3d_grad_finalize_abort(void);

/* ---- data-parallel exchange: RCCL over xGMI behind the ABI (one process per GPU) -----------------------------------------
 * The reference trains on one device (multi_view_model/train.py:21,35); the batch shards over ranks and the flat fp32 gradient
 * buffer is summed across them.  RCCL is looked up in the process image at run time (the host program's own
 * librccl / HIP runtime); without it every call returns MV3D_E_UNSUPPORTED.  Rank 0 creates a 128-byte id
 * (mv3d_comm_unique_id) and hands it to the other ranks by any side channel (file, environment, TCP store); every rank then
 * calls mv3d_comm_init on its own device.  Collectives are in place on `stream`, fp32, SUM; counts are in elements.
 * reduce_scatter: send holds world * recv_count elements, rank r receives the sum of slice r; allgather is its inverse. */
typedef struct mv3d_comm mv3d_comm;
int mv3d_comm_available(void);
int mv3d_comm_unique_id(void* id128);
int mv3d_comm_init(mv3d_comm** out, int rank, int world, const void* id128);
int mv3d_comm_destroy(mv3d_comm* comm);
int mv3d_comm_allreduce_sum(mv3d_comm* comm, void* buf, int64_t count, void* stream);
int mv3d_comm_reduce_scatter_sum(mv3d_comm* comm, const void* send, void* recv, int64_t recv_count, void* stream);
int mv3d_comm_allgather(mv3d_comm* comm, const void* send, void* recv, int64_t send_count, void* stream);

/* ---- mesh-direct exchange: xGMI is a full mesh of point-to-point links, so a rank that PULLS its slice of every
 * peer's gradient buffer directly uses all seven links at once, where a ring collective is bound by one.  mv3d_ipc_export gives
 * the 64-byte hipIpc handle of the allocation that holds `ptr` and ptr's offset in it; a peer process maps it with
 * mv3d_ipc_open (base of the allocation; add the offset) and unmaps it with mv3d_ipc_close.  mv3d_mesh_reduce_sum writes
 * dst[i] = srcs[0][i] + ... + srcs[nsrc-1][i], added in that order (srcs: host array of device pointers, local or mapped;
 * dst may be one of them); mv3d_mesh_copy is the pull of an updated slice.  Ordering between ranks (nobody reads a buffer its
 * owner is still writing) is the caller's: parallel.MeshComm does it over the control plane. */
#define MV3D_MESH_MAX_RANKS 8
int mv3d_ipc_export(const void* ptr, void* handle64, int64_t* offset);
int mv3d_ipc_open(const void* handle64, void** base);
int mv3d_ipc_close(void* base);
int mv3d_mesh_reduce_sum(const void* const* srcs, int nsrc, void* dst, int64_t count, void* stream);
int mv3d_mesh_copy(void* dst, const void* src, int64_t count, void* stream);

/* ---- recorded plans: native replay of a fixed launch sequence (the step is static) ----------
 * Between mv3d_plan_begin() and mv3d_plan_end() every mv3d_* op call on this thread is RECORDED
 * (validated, not launched).  mv3d_plan_run() launches the recorded sequence on a stream in one
 * native call (no per-op Python/ctypes cost); it is capture-safe (hipGraph). */
typedef struct mv3d_plan mv3d_plan;
mv3d_plan* mv3d_plan_create(void);
void mv3d_plan_destroy(mv3d_plan* p);
int mv3d_plan_begin(mv3d_plan* p);
int mv3d_plan_end(void);
int mv3d_plan_size(const mv3d_plan* p);
int mv3d_plan_run(mv3d_plan* p, void* stream);
/* launches ops [begin, end) only: lets the host interleave other stream work (bucket all-reduces of
 * the data-parallel path) between segments of the recorded backward sequence */
int mv3d_plan_run_range(mv3d_plan* p, int begin, int end, void* stream);
/* Multi-stream runs.  Calls recorded between mv3d_plan_side(k > 0) and mv3d_plan_side(0) are "side work" of class k: they
 * depend on everything recorded before them and nothing recorded after them in the plan depends on them (the filter / bias
 * gradients of the reverse pass: only the optimiser reads them).  mv3d_plan_run_range_multi issues side class k on
 * side_streams[(k-1) % nside] behind an event on `stream` (a fork whenever a run of that class begins) and makes `stream`
 * wait for every side stream it used at the end of the range, so the filter gradients of a layer run concurrently with
 * the data gradients of the layers below it.  Side work must not share scratch memory with main work, nor classes on
 * different streams with each other.  nside == 0: everything on `stream`, as mv3d_plan_run_range. */
#define MV3D_MAX_SIDE 4
int mv3d_plan_side(int side);                  /* 0 = main, 1..MV3D_MAX_SIDE = side work class */
#define MV3D_RUN_NO_JOIN 1      /* the caller orders `stream` behind the side streams itself */
int mv3d_plan_run_range_multi(mv3d_plan* p, int begin, int end, void* stream, void* const* side_streams, int nside, int flags);
/* Per-launch timing for the roofline report: with profiling enabled, mv3d_plan_run brackets every
 * recorded launch with hipEventRecord on the launch stream (no host synchronisation);
 * mv3d_plan_profile_collect() synchronises once and folds all runs into per-op totals.
 * mv3d_plan_op_info returns the kernel label, the algorithmic FLOPs and HBM bytes of launch i
 * (formulas in DESIGN.md), the accumulated milliseconds and the number of timed runs. */
int mv3d_plan_profile(mv3d_plan* p, int enable);
int mv3d_plan_profile_collect(mv3d_plan* p);
/* bracket only the launches whose kernel label matches `name` (NULL: all): one label or a '|'-separated list, each entry
 * optionally ending in '*' for a prefix match -- a handful of events per step, cheap enough to leave on inside a timed region */
int mv3d_plan_profile_select(mv3d_plan* p, const char* name);
int mv3d_plan_profile_reset(mv3d_plan* p);
int mv3d_plan_op_info(const mv3d_plan* p, int i, const char** name, double* flops, double* bytes,
                      double* total_ms, int* runs);

/* Diagnostics: copies the in-kernel clock stamps of the pipelined convolution kernel (csrc/cconv.hip; written only when the
 * environment sets MV3D_DBG bit 32) to host memory: [256 workgroups][8 waves][64 events] uint64 (tools/cconv_stamps.py). */
int mv3d_debug_cconv_stamps(void* host_dst, size_t bytes);
/* the same for the pipelined filter-gradient kernel (cwgrad): [128 slabs][8 waves][64 events] of the workgroups with blockIdx.x == 0 */
int mv3d_debug_cwgrad_stamps(void* host_dst, size_t bytes);
/* the same for the row-band kernel of the thin input layers (thin.hip): [workgroup < 512][wave 4][16] uint64 */
int mv3d_debug_band_stamps(void* host_dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
