// Entry points of the dense convolutions / linear layers: cfp_conv2d_nhwc, _ex, _moments, the data gradients and
// cfp_upsample_cat_conv3x3.  conv2d_impl validates, fills ConvP, asks conv_route (conv_route.hip) and launches what the route says.
#include "conv_route.h"

extern "C" int cfp_layernorm(const void* in, int in_ld, const float* gamma, const float* beta, float eps,
                             const void* residual, int res_ld, void* out, int out_ld, int rows, int C, int dtype,
                             cfp_stream_t stream);

static int conv2d_impl(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                                  const void* residual, int res_ld, void* out, int out_ld, int B, int H, int W, int Cin,
                                  int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int act,
                                  int dtype, const float* ln_gamma, const float* ln_beta, float ln_eps,
                                  int per_image_weights, void* ws, size_t ws_bytes, cfp_stream_t stream, int dil,
                                  float* mom = nullptr, size_t mom_floats = 0, int* mom_nsplit = nullptr, int* mom_rps = nullptr) {
  CFP_REQUIRE(in && w && out, CFP_EINVAL, "cfp_conv2d_nhwc: null pointer");
  if (mom_nsplit) *mom_nsplit = 0;
  if (mom_rps) *mom_rps = 0;
  CFP_REQUIRE(dtype_ok(dtype), CFP_EINVAL, "cfp_conv2d_nhwc: bad dtype");
  const int ve = vec_elems(dtype);
  CFP_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && Ho > 0 && Wo > 0,
              CFP_ESHAPE, "cfp_conv2d_nhwc: non-positive dimension");
  CFP_REQUIRE(Cin % ve == 0 && in_ld % ve == 0 && in_ld >= Cin, CFP_ESHAPE,
              "cfp_conv2d_nhwc: Cin / in_ld must be multiples of the 16-byte vector");
  CFP_REQUIRE(Cout % ve == 0 && out_ld % ve == 0 && out_ld >= Cout, CFP_ESHAPE,
              "cfp_conv2d_nhwc: Cout / out_ld must be multiples of the 16-byte vector");
  CFP_REQUIRE(!residual || (res_ld % ve == 0 && res_ld >= Cout), CFP_ESHAPE, "cfp_conv2d_nhwc: bad res_ld");
  CFP_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out) && aligned16(residual) && aligned16(ws), CFP_EINVAL,
              "cfp_conv2d_nhwc: pointers must be 16-byte aligned");
  CFP_REQUIRE(dil >= 1 && (dil == 1 || (stride == 1 && !per_image_weights && !ln_gamma)), CFP_EINVAL, "cfp_conv2d_nhwc: bad input dilation");
  const long long Hd = (long long)(H - 1) * dil + 1, Wd = (long long)(W - 1) * dil + 1;      // zero-stuffed input size
  // (a data gradient may extend past the stuffed input: forward pixels the strided window never reached get a zero gradient)
  CFP_REQUIRE(dil > 1 || ((Ho - 1) * stride - pad_t + KH - 1 < Hd + KH && (Wo - 1) * stride - pad_l + KW - 1 < Wd + KW), CFP_ESHAPE,
              "cfp_conv2d_nhwc: output size inconsistent with input size");
  CFP_REQUIRE((long long)B * Ho * Wo < (1ll << 31) && (long long)KH * KW * Cin < (1ll << 31), CFP_ESHAPE,
              "cfp_conv2d_nhwc: problem too large");
  CFP_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), CFP_EINVAL, "cfp_conv2d_nhwc: ln_gamma / ln_beta must come together");
  CFP_REQUIRE(!ln_gamma || (aligned16(ln_gamma) && aligned16(ln_beta)), CFP_EINVAL, "cfp_conv2d_nhwc: LayerNorm parameters must be 16-byte aligned");
  ConvP p{};      // every field a kernel family does not use stays zero / null
  p.in = in; p.w = w; p.out = out; p.res = residual; p.scale = scale; p.shift = shift;
  p.in_ld = in_ld; p.out_ld = out_ld; p.res_ld = res_ld;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.KH = KH; p.KW = KW; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
  p.M = B * Ho * Wo; p.K = KH * KW * Cin; p.act = act; p.f16 = dtype == CFP_F16; p.dil = dil;
  p.pointwise = (KH == 1 && KW == 1 && stride == 1 && pad_t == 0 && pad_l == 0 && Ho == H && Wo == W && dil == 1) ? 1 : 0;
  p.ln_eps = ln_eps; p.probe = g_probe;
  ConvArgs a{};
  a.dtype = dtype;
  a.per_image = (per_image_weights & CFP_CONV_PER_IMAGE) != 0;
  a.w2 = (per_image_weights & CFP_CONV_W2) != 0;
  a.x3 = (per_image_weights & CFP_CONV_X3) != 0;
  a.in_flight = (per_image_weights & CFP_CONV_IN_FLIGHT) != 0;
  a.want_tickets = (per_image_weights & CFP_CONV_WS_TICKETS) != 0;
  a.ln = ln_gamma != nullptr;
  a.want_mom = mom && mom_nsplit && mom_rps && is16(dtype) && !residual && !ln_gamma && !a.per_image && act == CFP_ACT_NONE && dil == 1;
  a.mom_floats = mom_floats;
  a.ws_bytes = ws ? ws_bytes : 0;
  a.gen2_fits = dil == 1 && is16(dtype) && p.K <= 16384 && KH < 256 && KW < 256 &&
                ((long long)B * H * W + (long long)pad_t * W + pad_l) * in_ld * 2 < (1ll << 31) - 65536 &&      // 32-bit byte offsets into
                (long long)Cout * p.K * 2 < (1ll << 31) - 65536;                                                    // buffer descriptors
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  if (a.x3) {
    // float32 storage, split-precision matrix math: `w` is the pre-split operand of cfp_pack_w_x3 (conv_igemm_x3.hip)
    CFP_REQUIRE(dtype == CFP_F32 && dil == 1 && !a.w2 && !mom, CFP_EINVAL, "cfp_conv2d_nhwc: CFP_CONV_X3 is for float32 storage (forward convolutions)");
    CFP_REQUIRE(KH < 256 && KW < 256 && (long long)H * W * in_ld < (1ll << 31) && (long long)cdiv(p.K, 32) * 64 * Cout < (1ll << 40), CFP_ESHAPE,
                "cfp_conv2d_nhwc: problem too large for the f16x3 kernel");
  } else {
    CFP_REQUIRE(!a.w2 || (p.pointwise && is16(dtype) && !a.per_image && dil == 1 && !g_use_v1), CFP_EINVAL,
                "cfp_conv2d_nhwc: two-term weights (CFP_CONV_W2) are for 16-bit pointwise layers with shared weights");
    CFP_REQUIRE(!a.w2 || a.gen2_fits, CFP_ESHAPE, "cfp_conv2d_nhwc: two-term weights need the gen-2 kernel (tensor too large for 32-bit offsets)");
  }
  if (a.x3 || (a.gen2_fits && !g_use_v1))
    CFP_REQUIRE(aligned16(scale) && aligned16(shift), CFP_EINVAL, "cfp_conv2d_nhwc: scale / shift must be 16-byte aligned (read as 4-float vectors)");

  const ConvRoute r = conv_route(p, a);
  CFP_REQUIRE(!r.error, CFP_EHIP, r.error);
  ConvKernel k = r.first;
  if (k.family == ConvFamily::Halo || k.family == ConvFamily::HaloX3) {
    // these two may decline at launch (LDS does not fit, 2^31 workgroups): the route's GEMM then, unless the variant was forced
    const bool x3h = k.family == ConvFamily::HaloX3;
    int rc = x3h ? conv3x3_halo_x3_launch(k.variant, p, s) : conv3x3_halo_launch(k.variant, p, s);
    if (rc == 0) return cfp_check_launch("cfp_conv2d_nhwc");
    CFP_REQUIRE(!r.must_run, CFP_EHIP, x3h ? "cfp_conv2d_nhwc: the forced f16x3 halo variant cannot run this problem"
                                           : "cfp_conv2d_nhwc: the forced halo variant cannot run this problem");
    k = r.fallback;
  }
  const int rpb = a.per_image ? Ho * Wo : 0;
  if (r.ln == ConvLn::After) p.res = nullptr;      // the residual is added after the LayerNorm kernel
  if (r.ln == ConvLn::Tile || r.ln == ConvLn::Reduce) { p.ln_gamma = ln_gamma; p.ln_beta = ln_beta; }
  if (r.mom_rows > 0) { p.mom = mom; *mom_nsplit = cdiv(p.M, r.mom_rows); *mom_rps = r.mom_rows; }
  switch (k.family) {
    case ConvFamily::Chunk: {
      int rc = conv3x3_chunk_launch(k.variant, p, s);
      CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_conv2d_nhwc: chunk 3x3 kernel launch failed");
      return cfp_check_launch("cfp_conv2d_nhwc");
    }
    case ConvFamily::Direct: {
      int rc = conv3x3_launch(k.variant, p, s);
      CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_conv2d_nhwc: direct 3x3 kernel launch failed");
      return cfp_check_launch("cfp_conv2d_nhwc");
    }
    case ConvFamily::RowGemm:
      rowgemm_f32_launch(p, s);
      return cfp_check_launch("cfp_conv2d_nhwc");
    case ConvFamily::X3: {
      if (rpb > 0) { p.rows_per_batch = rpb; p.w_bstride = (long long)Cout * cdiv(p.K, 32) * 64; }
      // CFP_CONV_WS_TICKETS: the first CFP_CONV_TICKET_BYTES of `ws` are the caller's zeroed ticket area and the slabs follow; the
      // ticket area is never slab space, whether this launch takes tickets or not
      float* slabs = (float*)(a.want_tickets && r.splits > 1 ? (char*)ws + CFP_CONV_TICKET_BYTES : (char*)ws);
      int rc = igemm_x3_launch(k.variant, p, slabs, r.splits, s, r.tickets ? (unsigned*)ws : nullptr);
      CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_conv2d_nhwc: f16x3 kernel launch failed");
      if (r.splits > 1 && !r.tickets) splitk_reduce_launch(CFP_F32, p, slabs, r.splits, s);
      break;
    }
    case ConvFamily::Gen2: {
      if (a.w2) p.k2 = cdiv(p.K, 64);
      if (rpb > 0) { p.rows_per_batch = rpb; p.w_bstride = (long long)Cout * p.K; }
      const int splits = rpb > 0 ? 1 : r.splits;      // per-image weights run un-split
      int rc = igemm2_launch(k.variant, p, (float*)ws, splits, s);
      CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_conv2d_nhwc: gen-2 kernel launch failed");
      if (splits > 1) splitk_reduce_launch(dtype, p, (const float*)ws, splits, s);
      break;
    }
    default: {      // Gen1: per-image weights run image by image
      const int nimg = a.per_image ? B : 1;
      const size_t esz = is16(dtype) ? 2 : 4;
      for (int b = 0; b < nimg; ++b) {
        ConvP q = p;
        if (a.per_image) {
          q.B = 1; q.M = Ho * Wo;
          q.in = (const char*)in + (size_t)b * H * W * in_ld * esz;
          q.out = (char*)out + (size_t)b * Ho * Wo * out_ld * esz;
          if (q.res) q.res = (const char*)q.res + (size_t)b * Ho * Wo * res_ld * esz;
          q.w = (const char*)w + (size_t)b * Cout * p.K * esz;
        }
        igemm1_launch(k.variant, dtype, q, (float*)ws, r.splits, s);
      }
      break;
    }
  }
  int e = cfp_check_launch("cfp_conv2d_nhwc");
  if (e != CFP_OK || r.ln != ConvLn::After) return e;
  return cfp_layernorm(out, out_ld, ln_gamma, ln_beta, ln_eps, residual, res_ld, out, out_ld, p.M, Cout, dtype, stream);
}

extern "C" int cfp_conv2d_nhwc_ex(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                                  const void* residual, int res_ld, void* out, int out_ld, int B, int H, int W, int Cin,
                                  int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int act,
                                  int dtype, const float* ln_gamma, const float* ln_beta, float ln_eps,
                                  int per_image_weights, void* ws, size_t ws_bytes, cfp_stream_t stream) {
  return conv2d_impl(in, in_ld, w, scale, shift, residual, res_ld, out, out_ld, B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo,
                     act, dtype, ln_gamma, ln_beta, ln_eps, per_image_weights, ws, ws_bytes, stream, 1);
}

// cfp_conv2d_nhwc + the per-row-tile channel moments of its (rounded, stored) output for a batch-statistics BatchNorm that follows
// (training: timm / torch `conv -> BatchNorm2d` in model.train()).  mom: [row tiles][2][Cout] float32 (mean, M2 about it); on return
// *nsplit = row tiles written (0: this problem's kernel does not produce them -- run cfp_bn_train_stats) and *rows_per_split = rows
// per tile; feed them to cfp_bn_train_stats_partials.
extern "C" int cfp_conv2d_nhwc_moments(const void* in, int in_ld, const void* w, const float* bias, void* out, int out_ld, int B, int H, int W,
                                       int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int dtype,
                                       void* ws, size_t ws_bytes, float* mom, size_t mom_floats, int* nsplit, int* rows_per_split,
                                       cfp_stream_t stream) {
  CFP_REQUIRE(mom && nsplit && rows_per_split, CFP_EINVAL, "cfp_conv2d_nhwc_moments: null moments pointer");
  return conv2d_impl(in, in_ld, w, nullptr, bias, nullptr, 0, out, out_ld, B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo,
                     CFP_ACT_NONE, dtype, nullptr, nullptr, 0.f, 0, ws, ws_bytes, stream, 1, mom, mom_floats, nsplit, rows_per_split);
}

int conv3x3_up_launch(int v, const ConvP& p, hipStream_t s);      // conv3x3_direct.hip

// UpSampleBN's first half in one launch (decoder.py:51-58): F.interpolate(low, size=(H, W), bilinear, align_corners=True) -> cat([up, skip],
// dim=1) -> conv3x3 (+ folded BatchNorm + activation).  Neither the upsampled tensor nor the concatenation exists in memory: the direct
// 3x3 kernel computes the upsampled channel chunks into its LDS halo tile and fetches the skip chunks.  Bit-identical to
// cfp_resize_bilinear + cfp_conv2d_nhwc on the concatenation buffer.  -> CFP_ESHAPE when the shape is not taken (caller keeps the pair).
extern "C" int cfp_upsample_cat_conv3x3(const void* low, int low_ld, int Hs, int Ws, int Cup, const void* skip, int skip_ld, int Cskip,
                                        const void* w, const float* scale, const float* shift, void* out, int out_ld, int B, int H, int W,
                                        int Cout, int act, int dtype, cfp_stream_t stream) {
  CFP_REQUIRE(low && skip && w && out, CFP_EINVAL, "cfp_upsample_cat_conv3x3: null pointer");
  if (dtype == CFP_F32X3) {
    // float32 tensors, f16x3 matrix math (round 5): the chunk-pipelined kernel with two sources (conv3x3_halo_x3.hip, UP = true).  `w` is the
    // pre-split operand packed over the PADDED channel axis [Cout][9][Cup + 32 ceil(Cskip / 32)] (ops.pack_w_x3_cat)
    CFP_REQUIRE(B > 0 && H > 1 && W > 1 && Hs > 0 && Ws > 0 && Cup > 0 && Cup % 32 == 0 && Cskip >= 4 && Cskip % 4 == 0 && Cout % 4 == 0 && Cout > 0 &&
                    low_ld % 4 == 0 && low_ld >= Cup && skip_ld % 4 == 0 && skip_ld >= Cskip && out_ld % 4 == 0 && out_ld >= Cout, CFP_ESHAPE,
                "cfp_upsample_cat_conv3x3 (f32x3): need Cup % 32 == 0, Cskip % 4 == 0 and 16-byte channel vectors");
    CFP_REQUIRE(aligned16(low) && aligned16(skip) && aligned16(w) && aligned16(out) && aligned16(scale) && aligned16(shift), CFP_EINVAL,
                "cfp_upsample_cat_conv3x3: pointers must be 16-byte aligned");
    CFP_REQUIRE(((long long)H * W) * skip_ld < (1ll << 31) - 65536 && ((long long)Hs * Ws) * low_ld < (1ll << 31) - 65536 && (long long)B * H * W < (1ll << 31),
                CFP_ESHAPE, "cfp_upsample_cat_conv3x3: tensor too large for 32-bit offsets");
    ConvP p{};
    p.in = skip; p.w = w; p.out = out; p.scale = scale; p.shift = shift;
    p.in_ld = skip_ld; p.out_ld = out_ld;
    p.B = B; p.H = H; p.W = W; p.Cin = Cup + Cskip; p.Ho = H; p.Wo = W; p.Cout = Cout;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad_t = 1; p.pad_l = 1;
    p.M = B * H * W; p.K = 9 * (Cup + cdiv(Cskip, 32) * 32); p.act = act; p.dil = 1;
    p.up_src = low; p.up_ld = low_ld; p.up_C = Cup; p.up_H = Hs; p.up_W = Ws;
    p.up_sy = (float)(Hs - 1) / (float)(H - 1);        // cfp_resize_bilinear's own expression
    p.up_sx = (float)(Ws - 1) / (float)(W - 1);
    int rc = conv3x3_halo_x3_launch(up_cat_x3_variant(Cout), p, reinterpret_cast<hipStream_t>(stream));
    CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_upsample_cat_conv3x3 (f32x3): kernel launch failed");
    return cfp_check_launch("cfp_upsample_cat_conv3x3");
  }
  CFP_REQUIRE(is16(dtype), CFP_ESHAPE, "cfp_upsample_cat_conv3x3: bf16 / f16 storage or CFP_F32X3");
  CFP_REQUIRE(B > 0 && H > 1 && W > 1 && Hs > 0 && Ws > 0 && Cup > 0 && Cup % 64 == 0 && Cskip > 0 && Cskip % 8 == 0 && Cout % 8 == 0 &&
                  low_ld % 8 == 0 && low_ld >= Cup && skip_ld % 8 == 0 && skip_ld >= Cskip && out_ld % 8 == 0 && out_ld >= Cout, CFP_ESHAPE,
              "cfp_upsample_cat_conv3x3: need Cup % 64 == 0 and 16-byte channel vectors");
  CFP_REQUIRE(aligned16(low) && aligned16(skip) && aligned16(w) && aligned16(out), CFP_EINVAL, "cfp_upsample_cat_conv3x3: pointers must be 16-byte aligned");
  const int Cin = Cup + Cskip;
  CFP_REQUIRE(((long long)B * H * W) * skip_ld * 2 < (1ll << 31) - 65536 && ((long long)Hs * Ws) * low_ld * 2 < (1ll << 31) - 65536 &&
                  (long long)Cout * 9 * Cin * 2 < (1ll << 31) - 65536 && (long long)B * H * W < (1ll << 31), CFP_ESHAPE,
              "cfp_upsample_cat_conv3x3: tensor too large for 32-bit offsets");
  ConvP p{};
  const size_t esz = 2;
  p.in = (const char*)skip - (size_t)Cup * esz;      // virtual base: channel c >= Cup of the concatenation is skip channel c - Cup
  p.w = w; p.out = out; p.scale = scale; p.shift = shift;
  p.in_ld = skip_ld; p.out_ld = out_ld;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Ho = H; p.Wo = W; p.Cout = Cout;
  p.KH = 3; p.KW = 3; p.stride = 1; p.pad_t = 1; p.pad_l = 1;
  p.M = B * H * W; p.K = 9 * Cin; p.act = act; p.f16 = dtype == CFP_F16; p.dil = 1;
  p.up_src = low; p.up_ld = low_ld; p.up_C = Cup; p.up_H = Hs; p.up_W = Ws;
  p.up_sy = (float)(Hs - 1) / (float)(H - 1);        // cfp_resize_bilinear's own expression (bit-identical source coordinates)
  p.up_sx = (float)(Ws - 1) / (float)(W - 1);
  // the whole-depth halo kernel where up_cat_halo_variant plans it (it may decline at launch), the 64-channel-chunk direct kernel otherwise
  const int hv = up_cat_halo_variant(p);
  if (hv >= -1) {
    int rc = conv3x3_halo_launch(hv, p, reinterpret_cast<hipStream_t>(stream));
    if (rc == 0) return cfp_check_launch("cfp_upsample_cat_conv3x3");
  }
  int rc = conv3x3_up_launch(up_cat_direct_variant(Cout), p, reinterpret_cast<hipStream_t>(stream));
  CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_upsample_cat_conv3x3: kernel launch failed");
  return cfp_check_launch("cfp_upsample_cat_conv3x3");
}

// Data gradient of a convolution: dX [B,H,W,Cin] from dY [B,Ho,Wo,Cout] and the flipped weights of cfp_conv2d_weight_flip
// ([Cin][KH][KW][Cout]).  dX = conv_stride1(zero-stuff(dY, stride), Wt) with padding K-1-pad, accumulate into dX when
// `accumulate` (the skip connections' gradient) by passing dX as the residual.
static int dgrad_x3(const float* dy, int dy_ld, const void* wt, const float* res, int res_ld, float* dx, int dx_ld, int B, int H, int W, int Cin,
                    int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, const int* dy_scale, void* ws, size_t ws_bytes,
                    cfp_stream_t stream);

extern "C" int cfp_conv2d_dgrad(const void* dy, int dy_ld, const void* wt, void* dx, int dx_ld, int B, int H, int W, int Cin, int Cout,
                                int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate, int dtype, void* ws,
                                size_t ws_bytes, cfp_stream_t stream) {
  CFP_REQUIRE(pad_t >= 0 && pad_l >= 0 && pad_t < KH && pad_l < KW, CFP_ESHAPE, "cfp_conv2d_dgrad: padding must be smaller than the kernel");
  if (dtype == CFP_F32X3)
    return dgrad_x3((const float*)dy, dy_ld, wt, accumulate ? (const float*)dx : nullptr, dx_ld, (float*)dx, dx_ld, B, H, W, Cin, Cout, KH, KW,
                    stride, pad_t, pad_l, Ho, Wo, nullptr, ws, ws_bytes, stream);
  return conv2d_impl(dy, dy_ld, wt, nullptr, nullptr, accumulate ? dx : nullptr, dx_ld, dx, dx_ld, B, Ho, Wo, Cout, Cin, KH, KW, 1,
                     KH - 1 - pad_t, KW - 1 - pad_l, H, W, CFP_ACT_NONE, dtype, nullptr, nullptr, 0.f, 0, ws, ws_bytes, stream, stride);
}

// f16x3 data gradient (float32 dY / dX, `wt` = the pre-split operand of the flipped weights, cfp_pack_w_x3_batch mode 1).  dY goes to the
// split-precision kernels of the forward either as it is (stride 1, no scale) or through cfp_grad_scale into `ws`: multiplied by the power of
// two of `dy_scale` and, for stride > 1, zero-stuffed (the x3 loaders take no input dilation: those few layers read a stuffed copy).  The
// convolution's per-channel epilogue scale is then 2^-e (exact), so dX comes out unscaled.
extern "C" size_t cfp_conv2d_dgrad_x3_ws_bytes(int B, int Ho, int Wo, int Cout, int Cin, int stride) {
  if (B <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0 || Cin <= 0 || stride <= 0) return 0;
  const long long Hd = (long long)(Ho - 1) * stride + 1, Wd = (long long)(Wo - 1) * stride + 1;
  return ((size_t)cdiv(Cin, 64) * 64 + (size_t)B * Hd * Wd * Cout) * sizeof(float);
}

static int dgrad_x3(const float* dy, int dy_ld, const void* wt, const float* res, int res_ld, float* dx, int dx_ld, int B, int H, int W, int Cin,
                    int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, const int* dy_scale, void* ws, size_t ws_bytes,
                    cfp_stream_t stream) {
  CFP_REQUIRE(pad_t >= 0 && pad_l >= 0 && pad_t < KH && pad_l < KW, CFP_ESHAPE, "cfp_conv2d_dgrad: padding must be smaller than the kernel");
  if (!dy_scale && stride == 1)
    return conv2d_impl(dy, dy_ld, wt, nullptr, nullptr, res, res_ld, dx, dx_ld, B, Ho, Wo, Cout, Cin, KH, KW, 1, KH - 1 - pad_t, KW - 1 - pad_l,
                       H, W, CFP_ACT_NONE, CFP_F32, nullptr, nullptr, 0.f, CFP_CONV_X3, nullptr, 0, stream, 1);
  CFP_REQUIRE(ws && aligned16(ws) && ws_bytes >= cfp_conv2d_dgrad_x3_ws_bytes(B, Ho, Wo, Cout, Cin, stride), CFP_EINVAL,
              "cfp_conv2d_dgrad (f16x3): workspace missing or too small (cfp_conv2d_dgrad_x3_ws_bytes)");
  float* inv = reinterpret_cast<float*>(ws);
  float* dys = inv + (size_t)cdiv(Cin, 64) * 64;
  int e = cfp_grad_scale(dy, dy_ld, B, Ho, Wo, Cout, stride, dy_scale, dys, inv, Cin, stream);
  if (e != CFP_OK) return e;
  const int Hd = (Ho - 1) * stride + 1, Wd = (Wo - 1) * stride + 1;
  return conv2d_impl(dys, Cout, wt, inv, nullptr, res, res_ld, dx, dx_ld, B, Hd, Wd, Cout, Cin, KH, KW, 1, KH - 1 - pad_t, KW - 1 - pad_l, H, W,
                     CFP_ACT_NONE, CFP_F32, nullptr, nullptr, 0.f, CFP_CONV_X3, nullptr, 0, stream, 1);
}

extern "C" int cfp_conv2d_dgrad_x3(const float* dy, int dy_ld, const void* wt, const float* res, int res_ld, float* dx, int dx_ld, int B, int H, int W,
                                   int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, const int* dy_scale,
                                   void* ws, size_t ws_bytes, cfp_stream_t stream) {
  return dgrad_x3(dy, dy_ld, wt, res, res_ld, dx, dx_ld, B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, dy_scale, ws, ws_bytes, stream);
}

extern "C" int cfp_conv2d_nhwc(const void* in, int in_ld, const void* w, const float* scale, const float* shift,
                               const void* residual, int res_ld, void* out, int out_ld, int B, int H, int W, int Cin,
                               int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int act,
                               int dtype, void* ws, size_t ws_bytes, cfp_stream_t stream) {
  return cfp_conv2d_nhwc_ex(in, in_ld, w, scale, shift, residual, res_ld, out, out_ld, B, H, W, Cin, Cout, KH, KW, stride,
                            pad_t, pad_l, Ho, Wo, act, dtype, nullptr, nullptr, 0.f, 0, ws, ws_bytes, stream);
}
