// What the MeasureVAE executor (plan_measure.hip) reaches in sequence.hip besides the C-ABI entry points.
#pragma once
#include "common.h"
#include "attributes.h"

namespace arvae {

// arvae_embed_fwd (wide rows) with the beat RNN's constant input in the same launch; false: not that case
bool embed_fwd_with_beat(const int64_t *idx, const float *table, int32_t batch, int32_t steps, int32_t dim, int32_t vocab, int32_t time_major,
                         float *out, const BeatInput &beat, hipStream_t s, int *rc);
// arvae_tick_gi_fwd that also copies the tokens it reads
int tick_gi_fwd_copy(const float *g_small, const int64_t *tokens, const float *bias, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                     int32_t vocab, int32_t cols, float *gi, int64_t *copy_to, hipStream_t s);

}  // namespace arvae
