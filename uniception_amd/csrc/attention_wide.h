// Internal interface of the head_dim > 64 attention path (attention_wide.hip).  uc_attention_fwd / uc_attention_bwd hand every
// descriptor with D > 64 to the two entry functions; the fp32 verification kernels stay templates of attention.hip /
// attention_bwd.hip, which instantiate them at DMAX 96 behind the two launchers below.
#pragma once
#include "attention_wide_plan.h"

int uc_attention_fwd_wide(const uc_attention_desc& d, uc_stream_t stream);
int uc_attention_bwd_wide(const uc_attention_bwd_desc& d, uc_stream_t stream);

// defined in attention.hip / attention_bwd.hip (arguments already validated)
int uc_attention_f32_96_launch(const uc_attention_desc& d, const AttnWideFwdPlan& plan, uc_stream_t stream);
int uc_attention_bwd_f32_96_launch(const uc_attention_bwd_desc& d, const AttnWideBwdPlan& plan, uc_stream_t stream);
