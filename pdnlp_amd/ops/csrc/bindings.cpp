// Python bindings for the pdnlp_amd gfx950 kernel extension.

#include <torch/extension.h>

#include <optional>
#include <string>
#include <vector>

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps);
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd);
std::vector<torch::Tensor> embedding_ln_fwd(
    torch::Tensor ids, torch::Tensor type_ids, torch::Tensor pos_ids,
    torch::Tensor word, torch::Tensor pos, torch::Tensor type_,
    torch::Tensor w, torch::Tensor b, double eps);
std::vector<torch::Tensor> embedding_ln_bwd(
    torch::Tensor dy, torch::Tensor ids, torch::Tensor type_ids,
    torch::Tensor pos_ids, torch::Tensor word, torch::Tensor pos,
    torch::Tensor type_, torch::Tensor w, torch::Tensor mean,
    torch::Tensor rstd);
torch::Tensor masked_softmax_fwd(torch::Tensor scores, torch::Tensor mask,
                                 double scale);
torch::Tensor masked_softmax_bwd(torch::Tensor dy, torch::Tensor p);
torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor b);
std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor b);
torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor pre);
torch::Tensor col_sum(torch::Tensor x);
torch::Tensor gemm_tn(torch::Tensor A, torch::Tensor B);
std::vector<torch::Tensor> gemm_tn_colsum(torch::Tensor A, torch::Tensor B);
torch::Tensor gemm_nn(torch::Tensor A, torch::Tensor B);
torch::Tensor gemm_nn_add(torch::Tensor A, torch::Tensor B, torch::Tensor D);
torch::Tensor skinny_linear_fwd(torch::Tensor x, torch::Tensor w,
                                torch::Tensor b);
std::vector<torch::Tensor> skinny_linear_bwd(torch::Tensor dy, torch::Tensor x,
                                             torch::Tensor w, bool need_db);
std::vector<torch::Tensor> dropout_fwd(torch::Tensor x, double p,
                                       torch::Tensor seed_buf, long salt);
torch::Tensor dropout_bwd(torch::Tensor dy, torch::Tensor mask, double p);
void multi_tensor_sgd(std::vector<torch::Tensor> params,
                      std::vector<torch::Tensor> grads,
                      std::vector<torch::Tensor> bufs,
                      std::vector<torch::Tensor> masters, double lr,
                      double momentum, double weight_decay,
                      double grad_scale_inv, torch::Tensor found_inf,
                        std::optional<torch::Tensor> grad_coef);
torch::Tensor tanh_bwd(torch::Tensor dy, torch::Tensor pre);
std::vector<torch::Tensor> bias_dropout_residual_ln_fwd(
    torch::Tensor y, torch::Tensor bias, torch::Tensor res, torch::Tensor lnw,
    torch::Tensor lnb, double p, double eps, torch::Tensor seed_buf,
    long salt);
std::vector<torch::Tensor> bias_dropout_residual_ln_bwd(
    torch::Tensor dout, torch::Tensor xsum, torch::Tensor mask,
    torch::Tensor lnw, torch::Tensor mean, torch::Tensor rstd, double p);
std::vector<torch::Tensor> bias_dropout_residual_ln_bwd_nodb(
    torch::Tensor dout, torch::Tensor xsum, torch::Tensor mask,
    torch::Tensor lnw, torch::Tensor mean, torch::Tensor rstd, double p);
std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor labels);
torch::Tensor cross_entropy_bwd(torch::Tensor dloss, torch::Tensor logprobs,
                                torch::Tensor labels);
std::vector<torch::Tensor> cross_entropy_ignore_fwd(torch::Tensor logits,
                                                    torch::Tensor labels,
                                                    long ignore_index);
torch::Tensor cross_entropy_ignore_bwd(torch::Tensor dloss,
                                       torch::Tensor logprobs,
                                       torch::Tensor labels,
                                       torch::Tensor nvalid,
                                       long ignore_index);
void multi_tensor_adamw(std::vector<torch::Tensor> params,
                        std::vector<torch::Tensor> grads,
                        std::vector<torch::Tensor> exp_avgs,
                        std::vector<torch::Tensor> exp_avg_sqs,
                        std::vector<torch::Tensor> masters, double lr,
                        double beta1, double beta2, double eps,
                        double weight_decay, double bc1, double bc2,
                        double grad_scale_inv, torch::Tensor found_inf,
                        std::optional<torch::Tensor> grad_coef);
void multi_tensor_unscale(std::vector<torch::Tensor> grads,
                          torch::Tensor found_inf, double inv_scale);
void multi_tensor_sumsq(std::vector<torch::Tensor> tensors, torch::Tensor out,
                        bool accumulate, double max_norm,
                        std::optional<torch::Tensor> coef_out,
                        std::optional<torch::Tensor> norm_out);
void clip_coef_from_sumsq(torch::Tensor sumsq, double max_norm,
                          torch::Tensor coef_out, torch::Tensor norm_out);
void multi_tensor_scale_(std::vector<torch::Tensor> tensors,
                         torch::Tensor coef);
std::vector<torch::Tensor> gemm_nt_fwd(torch::Tensor A, torch::Tensor W,
                                       torch::Tensor bias, std::string act);
std::vector<torch::Tensor> flash_attn_qkv_fwd(torch::Tensor qkv,
                                              torch::Tensor mask, long nh,
                                              double scale, double p,
                                              torch::Tensor seed_buf,
                                              long salt);
torch::Tensor flash_attn_qkv_bwd(torch::Tensor dout, torch::Tensor qkv,
                                 torch::Tensor o, torch::Tensor lse,
                                 torch::Tensor mask, long nh, double scale,
                                 double p, torch::Tensor seed_buf, long salt);
std::vector<torch::Tensor> flash_attn_varlen_fwd(torch::Tensor qkv,
                                                 torch::Tensor cu_seqlens,
                                                 long max_seqlen, long nh,
                                                 double scale, double p,
                                                 torch::Tensor seed_buf,
                                                 long salt);
torch::Tensor flash_attn_varlen_bwd(torch::Tensor dout, torch::Tensor qkv,
                                    torch::Tensor o, torch::Tensor lse,
                                    torch::Tensor cu_seqlens, long max_seqlen,
                                    long nh, double scale, double p,
                                    torch::Tensor seed_buf, long salt);
long flash_attn_tilepack_max_items(long T, long B);
torch::Tensor flash_attn_tilepack_plan(torch::Tensor cu_seqlens, long T);
std::vector<torch::Tensor> flash_attn_tilepack_fwd(torch::Tensor qkv,
                                                   torch::Tensor plan,
                                                   long max_seqlen, long nh,
                                                   double scale, double p,
                                                   torch::Tensor seed_buf,
                                                   long salt);
torch::Tensor flash_attn_tilepack_bwd(torch::Tensor dout, torch::Tensor qkv,
                                      torch::Tensor o, torch::Tensor lse,
                                      torch::Tensor plan, long max_seqlen,
                                      long nh, double scale, double p,
                                      torch::Tensor seed_buf, long salt);
torch::Tensor flash_attn_tilepack_infer(torch::Tensor qkv, torch::Tensor plan,
                                        long max_seqlen, long nh, double scale,
                                        std::optional<torch::Tensor> out);
torch::Tensor bias_dropout_residual_ln_infer(
    torch::Tensor y, torch::Tensor bias, torch::Tensor res, torch::Tensor lnw,
    torch::Tensor lnb, double eps);
std::vector<torch::Tensor> cls_attn_fwd(torch::Tensor qkv,
                                        torch::Tensor cu_seqlens,
                                        long rows_out, long max_seqlen,
                                        long nh, double scale, double p,
                                        torch::Tensor seed_buf, long salt);
torch::Tensor cls_attn_infer(torch::Tensor qkv, torch::Tensor cu_seqlens,
                             long rows_out, long max_seqlen, long nh,
                             double scale);
torch::Tensor cls_attn_bwd(torch::Tensor dout, torch::Tensor qkv,
                           torch::Tensor o, torch::Tensor lse,
                           torch::Tensor cu_seqlens, long max_seqlen, long nh,
                           double scale, double p, torch::Tensor seed_buf,
                           long salt);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("embedding_ln_fwd", &embedding_ln_fwd);
  m.def("embedding_ln_bwd", &embedding_ln_bwd);
  m.def("masked_softmax_fwd", &masked_softmax_fwd);
  m.def("masked_softmax_bwd", &masked_softmax_bwd);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("col_sum", &col_sum);
  m.def("gemm_tn", &gemm_tn);
  m.def("gemm_tn_colsum", &gemm_tn_colsum);
  m.def("gemm_nn", &gemm_nn);
  m.def("gemm_nn_add", &gemm_nn_add);
  m.def("skinny_linear_fwd", &skinny_linear_fwd);
  m.def("skinny_linear_bwd", &skinny_linear_bwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_bwd", &dropout_bwd);
  // grad_coef: optional fp32[1] device clip coefficient (grad_clip.hip);
  // trailing and defaulted, the positional 9/14-argument forms still work
  m.def("multi_tensor_sgd", &multi_tensor_sgd, py::arg("params"),
        py::arg("grads"), py::arg("bufs"), py::arg("masters"), py::arg("lr"),
        py::arg("momentum"), py::arg("weight_decay"),
        py::arg("grad_scale_inv"), py::arg("found_inf"),
        py::arg("grad_coef") = py::none());
  m.def("tanh_bwd", &tanh_bwd);
  m.def("bias_dropout_residual_ln_fwd", &bias_dropout_residual_ln_fwd);
  m.def("bias_dropout_residual_ln_bwd", &bias_dropout_residual_ln_bwd);
  m.def("bias_dropout_residual_ln_bwd_nodb",
        &bias_dropout_residual_ln_bwd_nodb);
  m.def("cross_entropy_fwd", &cross_entropy_fwd);
  m.def("cross_entropy_bwd", &cross_entropy_bwd);
  m.def("cross_entropy_ignore_fwd", &cross_entropy_ignore_fwd);
  m.def("cross_entropy_ignore_bwd", &cross_entropy_ignore_bwd);
  m.def("multi_tensor_adamw", &multi_tensor_adamw, py::arg("params"),
        py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"),
        py::arg("masters"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("weight_decay"), py::arg("bc1"),
        py::arg("bc2"), py::arg("grad_scale_inv"), py::arg("found_inf"),
        py::arg("grad_coef") = py::none());
  m.def("multi_tensor_sumsq", &multi_tensor_sumsq, py::arg("tensors"),
        py::arg("out"), py::arg("accumulate"), py::arg("max_norm") = 0.0,
        py::arg("coef_out") = py::none(), py::arg("norm_out") = py::none());
  m.def("clip_coef_from_sumsq", &clip_coef_from_sumsq);
  m.def("multi_tensor_scale_", &multi_tensor_scale_);
  m.def("multi_tensor_unscale", &multi_tensor_unscale);
  m.def("gemm_nt_fwd", &gemm_nt_fwd);
  m.def("flash_attn_qkv_fwd", &flash_attn_qkv_fwd);
  m.def("flash_attn_qkv_bwd", &flash_attn_qkv_bwd);
  m.def("flash_attn_varlen_fwd", &flash_attn_varlen_fwd);
  m.def("flash_attn_varlen_bwd", &flash_attn_varlen_bwd);
  m.def("flash_attn_tilepack_max_items", &flash_attn_tilepack_max_items);
  m.def("flash_attn_tilepack_plan", &flash_attn_tilepack_plan);
  m.def("flash_attn_tilepack_fwd", &flash_attn_tilepack_fwd);
  m.def("flash_attn_tilepack_bwd", &flash_attn_tilepack_bwd);
  // forward-only (serving) forms: no lse/xsum/mask/mean/rstd, no fill launch
  m.def("flash_attn_tilepack_infer", &flash_attn_tilepack_infer,
        py::arg("qkv"), py::arg("plan"), py::arg("max_seqlen"), py::arg("nh"),
        py::arg("scale"), py::arg("out") = py::none());
  m.def("bias_dropout_residual_ln_infer", &bias_dropout_residual_ln_infer);
  // one query row per sequence (cls_attention.hip)
  m.def("cls_attn_fwd", &cls_attn_fwd);
  m.def("cls_attn_infer", &cls_attn_infer);
  m.def("cls_attn_bwd", &cls_attn_bwd);
}
