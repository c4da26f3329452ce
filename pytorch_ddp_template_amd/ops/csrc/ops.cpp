// Binding + routing layer for the in-tree HIP extension (gfx950).
//
// Exposes the op surface ops/native.py expects.  Dtype routing picks the
// bf16 MFMA kernels or the exact-f32 MFMA kernels; shape glue (K padding to
// the GEMM kernels' chunk granularity, the im2col fallback for the
// non-pow2-channel stem, weight rotation / zero-stuffing for strided conv
// dgrad) lives here so the kernels stay branch-free on the hot path.

#include <torch/extension.h>

#include <vector>

// ---- implemented in the .hip translation units ----
// elementwise.hip
torch::Tensor relu_fwd(torch::Tensor x);
torch::Tensor relu_bwd(torch::Tensor dy, torch::Tensor y);
torch::Tensor add_relu_fwd(torch::Tensor a, torch::Tensor b);
torch::Tensor add_(torch::Tensor a, torch::Tensor b);
torch::Tensor gelu_fwd(torch::Tensor x);
torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x);
torch::Tensor col_sum(torch::Tensor dy);
torch::Tensor transpose2d(torch::Tensor x);
torch::Tensor avgpool_global(torch::Tensor x);
torch::Tensor avgpool_global_bwd(torch::Tensor dy, int64_t H, int64_t W);
std::vector<torch::Tensor> maxpool2d_fwd(torch::Tensor x, int64_t k, int64_t s,
                                         int64_t p);
torch::Tensor maxpool2d_bwd(torch::Tensor dy, torch::Tensor idx, int64_t H,
                            int64_t W);
torch::Tensor weight_rot(torch::Tensor w);
torch::Tensor zero_stuff(torch::Tensor dy, int64_t s, int64_t opad_h,
                         int64_t opad_w);
torch::Tensor im2col(torch::Tensor x, int64_t R, int64_t S, int64_t stride,
                     int64_t pad, int64_t Kpad);
// gemm_bf16.hip
torch::Tensor bmm_nt_bf16(torch::Tensor A, torch::Tensor B,
                          c10::optional<torch::Tensor> bias, bool relu);
// transposed-operand split-K NT (gemm_plain.hip): dw = A[I,M] @ B[J,M]^T,
// fp32 out, for linear/1x1-conv weight grads routed via explicit transposes
torch::Tensor gemm_nt_splitk_f32(torch::Tensor A, torch::Tensor B);
torch::Tensor bmm_tn_bf16(torch::Tensor A, torch::Tensor B);
std::vector<torch::Tensor> bmm_tn_bias_bf16(torch::Tensor A, torch::Tensor B);
torch::Tensor conv2d_fwd_bf16(torch::Tensor x, torch::Tensor w,
                              c10::optional<torch::Tensor> bias, int64_t stride,
                              int64_t pad, bool relu);
torch::Tensor conv2d_wgrad_bf16(torch::Tensor dy, torch::Tensor x,
                                int64_t stride, int64_t pad, int64_t R,
                                int64_t S);
torch::Tensor conv2d_dgrad_bf16(torch::Tensor dy, torch::Tensor wr,
                                int64_t stride, int64_t pad, int64_t H,
                                int64_t W,
                                c10::optional<torch::Tensor> addend,
                                c10::optional<torch::Tensor> addend_mask,
                                c10::optional<torch::Tensor> out_mask);
std::vector<torch::Tensor> conv2d_fwd_stats_bf16(
    torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias,
    int64_t stride, int64_t pad, bool relu);
std::vector<torch::Tensor> conv2d_dgrad_bnstats_bf16(
    torch::Tensor dy, torch::Tensor wr, int64_t stride, int64_t pad, int64_t H,
    int64_t W, torch::Tensor out_mask, torch::Tensor bn_x,
    torch::Tensor bn_mean, torch::Tensor bn_rstd);
// conv_glds.hip: does a conv shape take the halo-resident 64-wide tile
bool conv_halo64_eligible(int64_t H, int64_t W, int64_t C, int64_t Kout,
                          int64_t R, int64_t S, int64_t stride, int64_t pad);
// conv_glds.hip: the same for the halo-resident 128-wide tile (C = 128)
bool conv_halo128_eligible(int64_t H, int64_t W, int64_t C, int64_t Kout,
                           int64_t R, int64_t S, int64_t stride, int64_t pad);
// conv_glds.hip: does a conv's dgrad take the parity-split stride-2 route
// (arguments are the forward conv's: input H x W, Cin, Kout, batch N)
bool conv_dgrad_s2_parity_eligible(int64_t H, int64_t W, int64_t Cin,
                                   int64_t Kout, int64_t R, int64_t S,
                                   int64_t stride, int64_t pad, int64_t N);
// gemm_bf16.hip: does a 16-bit conv's wgrad take the patch-staged seg kernel
bool conv_wgrad_patch_eligible(int64_t H, int64_t W, int64_t Cin,
                               int64_t Kout, int64_t R, int64_t S,
                               int64_t stride, int64_t pad);
// gemm_f32.hip
torch::Tensor bmm_nt_f32(torch::Tensor A, torch::Tensor B,
                         c10::optional<torch::Tensor> bias, bool relu);
torch::Tensor bmm_tn_f32(torch::Tensor A, torch::Tensor B);
torch::Tensor conv2d_fwd_f32(torch::Tensor x, torch::Tensor w,
                             c10::optional<torch::Tensor> bias, int64_t stride,
                             int64_t pad, bool relu);
torch::Tensor conv2d_wgrad_f32(torch::Tensor dy, torch::Tensor x,
                               int64_t stride, int64_t pad, int64_t R,
                               int64_t S);
// norm.hip
std::vector<torch::Tensor> bn_fwd(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta,
                                  c10::optional<torch::Tensor> running_mean,
                                  c10::optional<torch::Tensor> running_var,
                                  double momentum, double eps, bool relu);
std::vector<torch::Tensor> bn_fwd_ws(torch::Tensor x, torch::Tensor gamma,
                                     torch::Tensor beta, torch::Tensor ws,
                                     c10::optional<torch::Tensor> running_mean,
                                     c10::optional<torch::Tensor> running_var,
                                     double momentum, double eps, bool relu,
                                     c10::optional<torch::Tensor> addend);
torch::Tensor bn_infer(torch::Tensor x, torch::Tensor gamma, torch::Tensor beta,
                       torch::Tensor rmean, torch::Tensor rvar, double eps,
                       bool relu);
std::vector<torch::Tensor> bn_bwd(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor gamma, torch::Tensor mean,
                                  torch::Tensor rstd,
                                  c10::optional<torch::Tensor> y_relu);
std::vector<torch::Tensor> bn_bwd_ws(torch::Tensor dy, torch::Tensor x,
                                     torch::Tensor gamma, torch::Tensor mean,
                                     torch::Tensor rstd, torch::Tensor ws);
std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor gamma,
                                         torch::Tensor beta, double eps);
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor gamma,
                                         torch::Tensor mean,
                                         torch::Tensor rstd);
torch::Tensor softmax_fwd(torch::Tensor x, double scale);
torch::Tensor softmax_bwd(torch::Tensor dy, torch::Tensor y, double scale);
// loss.hip
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor target);
torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor target,
                     torch::Tensor lse, torch::Tensor dloss);
torch::Tensor mse_fwd(torch::Tensor p, torch::Tensor t);
torch::Tensor mse_bwd(torch::Tensor p, torch::Tensor t, torch::Tensor dloss);
// attention.hip
std::vector<torch::Tensor> qkv_unpack(torch::Tensor qkv, int64_t heads);
torch::Tensor qkv_pack(torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                       int64_t N, int64_t heads);
torch::Tensor head_split(torch::Tensor x, int64_t heads);
std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t heads,
                                    double scale, bool want_p);
torch::Tensor attn_bwd(torch::Tensor qkv, torch::Tensor dout,
                       torch::Tensor out, torch::Tensor stats, int64_t heads,
                       double scale);
// multi_tensor.hip
void sgd_step(std::vector<torch::Tensor> params,
              std::vector<torch::Tensor> grads,
              std::vector<torch::Tensor> moms,
              std::vector<torch::Tensor> masters, double lr, double momentum,
              double wd, double damp, bool nesterov,
              c10::optional<torch::Tensor> guard,
              c10::optional<torch::Tensor> skip_count,
              c10::optional<torch::Tensor> lr_tensor);
void adamw_step(std::vector<torch::Tensor> params,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> exp_avgs,
                std::vector<torch::Tensor> exp_avg_sqs,
                std::vector<torch::Tensor> masters, double lr, double beta1,
                double beta2, double eps, double wd, torch::Tensor step,
                c10::optional<torch::Tensor> guard,
                c10::optional<torch::Tensor> skip_count,
                c10::optional<torch::Tensor> lr_tensor);
torch::Tensor l2norm_sq(std::vector<torch::Tensor> grads);
void scale_(std::vector<torch::Tensor> ts, double s);
void scale_by_tensor_(std::vector<torch::Tensor> ts, torch::Tensor s);
// dropout.hip: out = (res or 0) + x * elem mask * row mask, Philox in-kernel
torch::Tensor dropout_fwd(torch::Tensor x, c10::optional<torch::Tensor> res,
                          c10::optional<torch::Tensor> out, torch::Tensor step,
                          int64_t key0, int64_t key1, int64_t call_id_elem,
                          int64_t call_id_row, double p_elem, double p_row,
                          int64_t inner);
int64_t dropout_grid_cap();
int64_t dropout_block();

// ======================= routing helpers =================================

namespace {

bool is_bf16(const torch::Tensor& t) {
  // both 16-bit dtypes route to the (templated) 16-bit MFMA kernels
  return t.scalar_type() == torch::kBFloat16 ||
         t.scalar_type() == torch::kHalf;
}

int k_granule(const torch::Tensor& t) { return is_bf16(t) ? 8 : 4; }

// pad the trailing (K) dim up to the kernel's chunk granularity
torch::Tensor pad_k(const torch::Tensor& t, int mult) {
  long long K = t.size(-1);
  long long pad = (mult - K % mult) % mult;
  if (pad == 0) return t;
  return torch::constant_pad_nd(t, {0, pad});
}

bool pow2_ge(int v, int lo) {
  return v >= lo && (v & (v - 1)) == 0;
}

}  // namespace

// C = A @ B^T (+bias)(+relu); A [.., M, K], B [N, K]
torch::Tensor gemm_nt(torch::Tensor A, torch::Tensor B,
                      c10::optional<torch::Tensor> bias, bool relu,
                      bool /*out_f32_unused*/) {
  TORCH_CHECK(A.scalar_type() == B.scalar_type(), "dtype mismatch");
  int g = k_granule(A);
  if (A.size(-1) % g) {
    A = pad_k(A.contiguous(), g);
    B = pad_k(B.contiguous(), g);
  }
  if (is_bf16(A)) return bmm_nt_bf16(A.contiguous(), B.contiguous(), bias, relu);
  return bmm_nt_f32(A.contiguous(), B.contiguous(), bias, relu);
}

torch::Tensor gemm_tn(torch::Tensor A, torch::Tensor B) {
  if (is_bf16(A)) return bmm_tn_bf16(A.contiguous(), B.contiguous());
  return bmm_tn_f32(A.contiguous(), B.contiguous());
}

torch::Tensor bmm_nt(torch::Tensor A, torch::Tensor B) {
  int g = k_granule(A);
  if (A.size(-1) % g) {
    A = pad_k(A.contiguous(), g);
    B = pad_k(B.contiguous(), g);
  }
  if (is_bf16(A)) return bmm_nt_bf16(A.contiguous(), B.contiguous(), {}, false);
  return bmm_nt_f32(A.contiguous(), B.contiguous(), {}, false);
}

torch::Tensor bmm_tn(torch::Tensor A, torch::Tensor B) {
  auto C = is_bf16(A) ? bmm_tn_bf16(A.contiguous(), B.contiguous())
                      : bmm_tn_f32(A.contiguous(), B.contiguous());
  return C.to(A.scalar_type());
}

// C[b,M,N] = A[b,M,K] @ B[b,K,N]: realized as NT against B^T (fast batched
// LDS transpose, then the NT MFMA kernel).
torch::Tensor bmm_nn(torch::Tensor A, torch::Tensor B) {
  auto Bt = transpose2d(B.contiguous());  // [b, N, K]
  return bmm_nt(A, Bt);
}

// ---- conv2d ----

torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias, int64_t stride,
                         int64_t pad, bool relu) {
  int Cin = (int)x.size(3);
  int R = (int)w.size(1), S = (int)w.size(2), Kout = (int)w.size(0);
  const bool fast = is_bf16(x) ? pow2_ge(Cin, 8) : pow2_ge(Cin, 4);
  if (fast) {
    if (is_bf16(x))
      return conv2d_fwd_bf16(x.contiguous(), w.contiguous(), bias, stride, pad,
                             relu);
    return conv2d_fwd_f32(x.contiguous(), w.contiguous(), bias, stride, pad,
                          relu);
  }
  // generic fallback: explicit im2col + NT GEMM (used by the 3-channel stem)
  int K = R * S * Cin;
  int g = k_granule(x);
  int Kpad = (K + g - 1) / g * g;
  auto cols = im2col(x.contiguous(), R, S, stride, pad, Kpad);
  auto wf = pad_k(w.contiguous().reshape({Kout, K}), g);
  auto y = is_bf16(x) ? bmm_nt_bf16(cols, wf.contiguous(), bias, relu)
                      : bmm_nt_f32(cols, wf.contiguous(), bias, relu);
  int N = (int)x.size(0), H = (int)x.size(1), W = (int)x.size(2);
  int HO = (H + 2 * (int)pad - R) / (int)stride + 1;
  int WO = (W + 2 * (int)pad - S) / (int)stride + 1;
  return y.reshape({N, HO, WO, Kout});
}

torch::Tensor conv2d_dgrad(torch::Tensor dy, torch::Tensor w, int64_t stride,
                           int64_t pad, int64_t H, int64_t W,
                           c10::optional<torch::Tensor> addend,
                           c10::optional<torch::Tensor> addend_mask,
                           c10::optional<torch::Tensor> out_mask) {
  // dx = conv(zero_stuffed(dy), rot(w), stride=1, pad=R-1-pad); output
  // padding covers (H+2p-R) % stride != 0 (inputs the fwd never reached).
  // Full contract: dx = relu_bwd(dgrad + masked(addend), out_mask), each
  // part optional, whichever kernel runs.
  int R = (int)w.size(1), S = (int)w.size(2);
  TORCH_CHECK(pad <= R - 1 && pad <= S - 1, "dgrad needs pad <= kernel-1");
  auto wr = weight_rot(w.contiguous());  // [C, R, S, Kout]
  int Kout = (int)dy.size(3);
  if (is_bf16(dy) ? pow2_ge(Kout, 8) : false) {
    // bf16/f16 fast path: zero-stuffing folded into the GEMM's im2col
    // gather (never materialized) — gemm_bf16.hip conv2d_dgrad_bf16.
    return conv2d_dgrad_bf16(dy.contiguous(), wr, stride, pad, H, W, addend,
                             addend_mask, out_mask);
  }
  int64_t opad_h = (H + 2 * pad - R) % stride;
  int64_t opad_w = (W + 2 * pad - S) % stride;
  auto dys = stride > 1 ? zero_stuff(dy.contiguous(), stride, opad_h, opad_w)
                        : dy.contiguous();
  auto dx = conv2d_fwd(dys, wr, {}, 1, R - 1 - pad, false);
  if (addend.has_value()) {
    auto a = *addend;
    if (addend_mask.has_value())
      a = a * (addend_mask->reshape(a.sizes()) > 0).to(a.scalar_type());
    dx = dx + a.reshape(dx.sizes());
  }
  if (out_mask.has_value())
    dx = torch::where(out_mask->reshape(dx.sizes()) > 0, dx,
                      torch::zeros_like(dx));
  TORCH_CHECK(dx.size(1) == H && dx.size(2) == W,
              "dgrad shape mismatch: got ", dx.sizes(), " want H=", H, " W=",
              W, " (input H+2p-R must be divisible by stride)");
  return dx;
}

// conv2d_dgrad(..., out_mask=out_mask) that, when the glds kernel takes the
// call, also returns the BN-backward sums workspace of the BN with input
// bn_x, saved bn_mean / bn_rstd and ReLU output out_mask (for bn_bwd_ws).
// Every other route returns the same masked dx and None.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> conv2d_dgrad_bnstats(
    torch::Tensor dy, torch::Tensor w, int64_t stride, int64_t pad, int64_t H,
    int64_t W, torch::Tensor out_mask, torch::Tensor bn_x,
    torch::Tensor bn_mean, torch::Tensor bn_rstd) {
  int R = (int)w.size(1), S = (int)w.size(2);
  TORCH_CHECK(pad <= R - 1 && pad <= S - 1, "dgrad needs pad <= kernel-1");
  if (is_bf16(dy) && pow2_ge((int)dy.size(3), 8)) {
    auto wr = weight_rot(w.contiguous());  // [C, R, S, Kout]
    auto r = conv2d_dgrad_bnstats_bf16(dy.contiguous(), wr, stride, pad, H, W,
                                       out_mask, bn_x, bn_mean, bn_rstd);
    if (r.size() == 2) return {r[0], r[1]};
    return {r[0], c10::nullopt};
  }
  return {conv2d_dgrad(dy, w, stride, pad, H, W, c10::nullopt, c10::nullopt,
                       out_mask),
          c10::nullopt};
}

torch::Tensor conv2d_wgrad(torch::Tensor dy, torch::Tensor x, int64_t stride,
                           int64_t pad, int64_t R, int64_t S) {
  int Cin = (int)x.size(3);
  const bool fast = is_bf16(x) ? pow2_ge(Cin, 8) : pow2_ge(Cin, 4);
  dy = dy.contiguous();
  x = x.contiguous();
  if (fast) {
    return is_bf16(x) ? conv2d_wgrad_bf16(dy, x, stride, pad, R, S)
                      : conv2d_wgrad_f32(dy, x, stride, pad, R, S);
  }
  // generic fallback: im2col + TN GEMM
  int K = (int)(R * S * Cin);
  int g = k_granule(x);
  int Kpad = (K + g - 1) / g * g;
  auto cols = im2col(x, R, S, stride, pad, Kpad);  // [M, Kpad]
  int Kout = (int)dy.size(3);
  auto dw = is_bf16(x)
                ? bmm_tn_bf16(dy.reshape({-1, Kout}).contiguous(), cols)
                : bmm_tn_f32(dy.reshape({-1, Kout}).contiguous(), cols);
  // [Kout, Kpad] f32 -> [Kout, R, S, Cin]
  return dw.narrow(1, 0, K).reshape({Kout, R, S, Cin}).contiguous();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gemm_nt", &gemm_nt, py::arg("A"), py::arg("B"),
        py::arg("bias") = c10::nullopt, py::arg("relu") = false,
        py::arg("out_f32") = false);
  m.def("gemm_tn", &gemm_tn);
  m.def("gemm_nt_splitk_f32", &gemm_nt_splitk_f32);
  m.def("gemm_tn_bias", [](torch::Tensor A, torch::Tensor B) {
    TORCH_CHECK(A.scalar_type() == torch::kBFloat16 ||
                A.scalar_type() == torch::kHalf,
                "gemm_tn_bias: 16-bit dtypes only");
    return bmm_tn_bias_bf16(A.contiguous(), B.contiguous());
  });
  m.def("bmm_nt", &bmm_nt);
  m.def("bmm_nn", &bmm_nn);
  m.def("bmm_tn", &bmm_tn);
  m.def("transpose2d", &transpose2d);
  m.def("conv2d_fwd", &conv2d_fwd, py::arg("x"), py::arg("w"),
        py::arg("bias") = c10::nullopt, py::arg("stride") = 1,
        py::arg("pad") = 0, py::arg("relu") = false);
  m.def("conv2d_dgrad", &conv2d_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("H"), py::arg("W"),
        py::arg("addend") = c10::nullopt,
        py::arg("addend_mask") = c10::nullopt,
        py::arg("out_mask") = c10::nullopt);
  m.def("conv2d_dgrad_bnstats", &conv2d_dgrad_bnstats, py::arg("dy"),
        py::arg("w"), py::arg("stride"), py::arg("pad"), py::arg("H"),
        py::arg("W"), py::arg("out_mask"), py::arg("bn_x"),
        py::arg("bn_mean"), py::arg("bn_rstd"));
  m.def("conv2d_fwd_stats", &conv2d_fwd_stats_bf16, py::arg("x"),
        py::arg("w"), py::arg("bias") = c10::nullopt, py::arg("stride") = 1,
        py::arg("pad") = 0, py::arg("relu") = false);
  m.def("conv_halo64_eligible", &conv_halo64_eligible, py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("Kout"), py::arg("R"),
        py::arg("S"), py::arg("stride"), py::arg("pad"));
  m.def("conv_halo128_eligible", &conv_halo128_eligible, py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("Kout"), py::arg("R"),
        py::arg("S"), py::arg("stride"), py::arg("pad"));
  m.def("conv_dgrad_s2_parity_eligible", &conv_dgrad_s2_parity_eligible,
        py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Kout"),
        py::arg("R"), py::arg("S"), py::arg("stride"), py::arg("pad"),
        py::arg("N"));
  m.def("conv_wgrad_patch_eligible", &conv_wgrad_patch_eligible,
        py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Kout"),
        py::arg("R"), py::arg("S"), py::arg("stride"), py::arg("pad"));
  m.def("conv2d_wgrad", &conv2d_wgrad);
  m.def("relu_fwd", &relu_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("add_relu_fwd", &add_relu_fwd);
  m.def("add_", &add_);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("col_sum", &col_sum);
  m.def("avgpool_global", &avgpool_global);
  m.def("avgpool_global_bwd", &avgpool_global_bwd);
  m.def("maxpool2d_fwd", &maxpool2d_fwd);
  m.def("maxpool2d_bwd", &maxpool2d_bwd);
  m.def("bn_fwd", &bn_fwd);
  m.def("bn_fwd_ws", &bn_fwd_ws, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("ws"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("relu"), py::arg("addend") = c10::nullopt);
  m.def("bn_infer", &bn_infer);
  m.def("bn_bwd", &bn_bwd, py::arg("dy"), py::arg("x"), py::arg("gamma"),
        py::arg("mean"), py::arg("rstd"), py::arg("y_relu") = c10::nullopt);
  m.def("bn_bwd_ws", &bn_bwd_ws, py::arg("dy"), py::arg("x"),
        py::arg("gamma"), py::arg("mean"), py::arg("rstd"), py::arg("ws"));
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("softmax_fwd", &softmax_fwd);
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("heads"),
        py::arg("scale"), py::arg("want_p") = false);
  m.def("attn_bwd", &attn_bwd);
  m.def("qkv_unpack", &qkv_unpack);
  m.def("qkv_pack", &qkv_pack);
  m.def("head_split", &head_split);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("mse_fwd", &mse_fwd);
  m.def("mse_bwd", &mse_bwd);
  m.def("sgd_step", &sgd_step, py::arg("params"), py::arg("grads"),
        py::arg("moms"), py::arg("masters"), py::arg("lr"),
        py::arg("momentum"), py::arg("wd"), py::arg("damp"),
        py::arg("nesterov"), py::arg("guard") = py::none(),
        py::arg("skip_count") = py::none(),
        py::arg("lr_tensor") = py::none());
  m.def("adamw_step", &adamw_step, py::arg("params"), py::arg("grads"),
        py::arg("exp_avgs"), py::arg("exp_avg_sqs"), py::arg("masters"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("step"), py::arg("guard") = py::none(),
        py::arg("skip_count") = py::none(),
        py::arg("lr_tensor") = py::none());
  m.def("l2norm_sq", &l2norm_sq);
  m.def("scale_", &scale_);
  m.def("scale_by_tensor_", &scale_by_tensor_);
  m.def("dropout_fwd", &dropout_fwd, py::arg("x"), py::arg("res"),
        py::arg("out"), py::arg("step"), py::arg("key0"), py::arg("key1"),
        py::arg("call_id_elem"), py::arg("call_id_row"), py::arg("p_elem"),
        py::arg("p_row"), py::arg("inner"));
  m.def("dropout_grid_cap", &dropout_grid_cap);
  m.def("dropout_block", &dropout_block);
  m.def("im2col", &im2col);
  m.def("weight_rot", &weight_rot);
  m.def("zero_stuff", &zero_stuff);
}
