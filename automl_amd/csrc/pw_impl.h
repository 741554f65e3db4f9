// The tuned bf16 implementations behind the pointwise / dense-convolution entry points, one family per file.  The dispatch
// (pw_gemm.hip, conv.hip) tries them in the order its routing rules give and falls back to the generic kernels.
// Every function here returns 1 = handled, 0 = the call lies outside its envelope (nothing was launched: the caller goes on
// to the next implementation), < 0 = error (edet_set_error has the text).
#pragma once
#include "common.h"

// ---- wave-private streaming kernels, weights resident in LDS (pw_stream_fwd / _dgrad / _wgrad / _fused.hip)
int pws_try_fwd(const edet_tview_t* in, const void* wt, int ldw, const float* bias, void* out, int cout,
                int ldo, float* stat_partials, int* nparts_out, hipStream_t st);
int pws_try_dgrad(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                  const edet_bwd_epi_t* epi, int* nparts_out, hipStream_t st);
int pws_try_wgrad(const edet_tview_t* in, const edet_gview_t* dy, float* dweight, void* workspace,
                  size_t workspace_bytes, hipStream_t st);
// both gradients in one pass; dweight [KO][R] fp32 is accumulated into
int pws_try_bwd_fused(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                      const edet_bwd_epi_t* epi, int* nparts_out, float* dweight, void* workspace,
                      size_t workspace_bytes, hipStream_t st);

// ---- workgroup-tiled kernels for the wide layers (pw_big.hip)
int pwb_try_fwd(const edet_tview_t* in, const void* wt, int ldw, const float* bias, void* out, int cout,
                int ldo, float* stat_partials, int* nparts_out, hipStream_t st);
// forward with fp32 output [rows][ldo] (ldo in floats, >= cout rounded up to 8); no statistics
int pwb_fwd_f32out(const edet_tview_t* in, const void* wt, int ldw, const float* bias, float* out, int cout, int ldo,
                   hipStream_t st);
int pwb_try_dgrad(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                  const edet_bwd_epi_t* epi, int* nparts_out, hipStream_t st);
int pwb_try_wgrad(const edet_tview_t* in, const edet_gview_t* dy, float* dweight, void* workspace,
                  size_t workspace_bytes, hipStream_t st);
// dense k x k convolution (stride s, TF 'SAME') as implicit GEMMs.  Forward: wt [cout][k*k*cin], reduction index
// (ky*k + kx)*cin + c contiguous.  Data gradient: w_t [cin][ldw], reduction index (ky*k + kx)*cout + co contiguous.
// Weight gradient: dweight fp32 HWIO [k][k][cin][cout] is accumulated into.
int pwb_try_conv_fwd(const edet_tview_t* in, const void* wt, int ldw, int k, int s, const float* bias, void* out,
                     int cout, int ldo, float* stat_partials, int* nparts_out, hipStream_t st);
int pwb_try_conv_dgrad(const edet_gview_t* dy, const void* w_t, int ldw, int k, int s, const edet_tview_t* in,
                       const edet_bwd_epi_t* epi, int* nparts_out, hipStream_t st);
int pwb_try_conv_wgrad(const edet_tview_t* in, const edet_gview_t* dy, int k, int s, float* dweight, void* workspace,
                       size_t workspace_bytes, hipStream_t st);

// ---- the LDS-DMA wide forward (pw_glds.hip); tpw = consecutive row tiles per workgroup, as pwb_try_fwd chose them
int pwg_try_fwd(const edet_tview_t* in, const void* wt, int ldw, const float* bias, void* out, int cout,
                int ldo, float* stat_partials, int* nparts_out, int tpw, hipStream_t st);

// ---- one-pass tiled data + weight gradient (pw_tile_bwd.hip)
int pwt_try_bwd(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in, const edet_bwd_epi_t* epi,
                int* nparts_out, float* dweight, void* workspace, size_t workspace_bytes, hipStream_t st);

// ---- 3 x 3 dense convolution forward with the input halo in LDS (conv_halo.hip)
int cvh_try_conv_fwd(const edet_tview_t* in, const void* wt, int ldw, int k, int s, void* out, int cout, int ldo,
                     float* stat_partials, int* nparts_out, hipStream_t st);
