// The two launchers of the bf16 head_dim 80 / 96 kernels (attention_wide.hip).  uc_attention_fwd / uc_attention_bwd have validated
// the descriptor and made the plan (attention_plan.h); a launcher fills the kernels' parameters and launches what the plan names.
#pragma once
#include "attention_plan.h"

int uc_attention_wide_fwd_launch(const uc_attention_desc& d, const AttnFwdPlan& plan, uc_stream_t stream);
int uc_attention_wide_bwd_launch(const uc_attention_bwd_desc& d, const AttnBwdPlan& plan, uc_stream_t stream);
