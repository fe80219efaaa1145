// What beam_decoder.hip offers the other files of the library: one tick's selection of the beam search on given logits
// (beam_select_kernel, through its launcher) and the checks that every beam search entry point makes of its width, mask and groups.
#pragma once
#include "common.h"

namespace arvae {

constexpr int BEAM_MAX_WIDTH = 16;

// beam_select_kernel on `stream`, one wave per code: logits [codes * width][vocab], scores_in / scores_out / parents / notes
// [codes][width]; allow null or the first code's mask, allow_stride bytes between the codes' masks (0: one mask); groups 1 and
// logp_in / logp_out null: not grouped.  Nothing is checked here: the entry points have checked.
void beam_select_launch(const float *logits, const float *scores_in, int codes, int width, int vocab, int live, const uint8_t *allow,
                        int64_t allow_stride, int *parents, int64_t *notes, float *scores_out, int groups, float penalty,
                        const float *logp_in, float *logp_out, hipStream_t stream);

// 1 <= width <= 16, the mask's count given by the host (the mask lives on the device) and at least `width` notes allowed, so that
// `width` distinct hypotheses exist after the first tick
int beam_width_check(const char *who, int32_t width, int32_t vocab, const uint8_t *allow, int32_t allowed);
// what the grouped entry points check of (width, groups, penalty)
int beam_groups_check(const char *who, int32_t width, int32_t groups, float penalty);

}  // namespace arvae
