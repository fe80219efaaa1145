// Diagnostic switches of the library.  The PRODUCT build reads no environment variable: diag_env() is the constant "not set",
// every switch below is dead code the compiler removes, and there is one code path per kernel family.  A DIAGNOSTIC build
// (-DARVAE_DIAG: ar-vae_amd/libarvae_hip_diag.so, built next to the product library and selected with ARVAE_LIB;
// tools/build_diag.sh for one-file variants) reads them, once per switch.  Every switch is held by a test to the default path
// it replaces:
//   ARVAE_NO_PAIR4, _NO_PAIR32, _NO_PAIR_C1, _NO_PAIR_TAIL, _NO_PAIR_PREP, _NO_PAIR_REG   paired launches apart
//                                         (tests/test_hip_parity.py test_paired_launches_match_the_separate_launches)
//   ARVAE_NO_DOWN_CHAIN                   the chained forward layers as two launches (test_chained_forward_layers_match_the_two_launches)
//   ARVAE_MIDBLOCK=0, ARVAE_MID_NO_CLUSTER, ARVAE_HEADS_NEXT   the latent block per layer / on its row kernels / heads riding the
//                                         next launch (test_latent_block_experiment_matches_the_per_layer_path)
//   ARVAE_GRU_WIDE, _GRU_BF16_BWD, _GRU_MASK_APART   the MeasureVAE recurrences as through round 4 (tests/test_measure_executor.py)
//   ARVAE_MIDC_DROP_ARRIVAL               one member of the latent block's first hand-off never arrives (the hand-off tests of
//                                         tests/test_hip_parity.py, through tests/shared_device_worker.py)
// DESIGN.md section 5 lists them.  The phase stamps (stamps.h: -DARVAE_STAMPS_<FAMILY>, tools/stamp.py) are compile-time instruments.
#pragma once
#include <stdlib.h>

namespace arvae {

#ifdef ARVAE_DIAG
inline const char *diag_env(const char *name) { return getenv(name); }
#else
constexpr const char *diag_env(const char *) { return nullptr; }
#endif

// compute units of the current device (queried once per process; 256 when the query fails)
int device_cu_count();

}  // namespace arvae
