// Phase stamps: the library's in-kernel timing instrument, defined here once.  A kernel family compiled with its flag records
// clock values at phase boundaries in a __device__ table; `tools/stamp.py <family>` runs the family's workload and prints the
// table.  One flag per family, armed one at a time (a stamp perturbs the kernel it measures: there is no "all" flag); neither the
// product nor the -DARVAE_DIAG library is built with any of them, and with no flag set this header declares nothing.
//
//   flag                  source (table in)          table [rows][slots][words]                       a stamp is
//   ARVAE_STAMPS_CONV32   conv32.hip                 conv32 [512 workgroups / roles][64][2]           {cycle counter, wall clock}
//   ARVAE_STAMPS_D32K     conv32.hip (down32p.h)     d32k   [2 roles x 32 workgroups][64][1]          wall clock
//   ARVAE_STAMPS_WGR      conv32.hip (wgrad32r.h)    wgr    [256 workgroups x 2 roles][64][2]         {cycle counter, wall clock}
//   ARVAE_STAMPS_C64S     conv64s.hip                c64s   [64 workgroups][64][1]                    wall clock
//   ARVAE_STAMPS_MIDC     midcluster.hip             midc   [2 passes x 256 workgroups][16][1]        wall clock
//   ARVAE_STAMPS_MID      midblock.hip               mid    [128 workgroups][16][1]                   wall clock
//   ARVAE_STAMPS_RG       dense.hip                  rg     [512 workgroups][32][1]                   wall clock
//   ARVAE_STAMPS_DW       dense.hip                  dw     [512 tiles][8][1]                         wall clock
//   ARVAE_STAMPS_S8       conv64.hip                 s8     7 phase sums + tiles per workgroup        cycles summed per phase
//   ARVAE_STAMPS_GRU      gru_seq.hip                gru    4 phase sums + steps                      cycles summed per phase
//   ARVAE_STAMPS_TICK     tick_decoder.hip           tick   8 phase sums + ticks                      cycles summed per phase
//   (-DGRU_STAMP_WAVE=w with GRU or TICK: wave w of workgroup 0 writes the sums instead of wave 0)
//
// Timeline families: ARVAE_STAMP_TABLE(family, rows, slots, words) declares the table and its reader; ARVAE_STAMP(table, row, slot)
// writes one stamp.  WHICH lane stamps and how a workgroup, role or pass maps to a row is the kernel's business: a one-line macro
// beside the kernel.  Phase-sum families: ARVAE_STAMP_TABLE(family, 1, N + 1, 1) and a PhaseSums<N> in the kernel.
#pragma once
#if defined(ARVAE_STAMPS_CONV32) || defined(ARVAE_STAMPS_D32K) || defined(ARVAE_STAMPS_WGR) || defined(ARVAE_STAMPS_C64S) || \
    defined(ARVAE_STAMPS_MIDC) || defined(ARVAE_STAMPS_MID) || defined(ARVAE_STAMPS_RG) || defined(ARVAE_STAMPS_DW) ||       \
    defined(ARVAE_STAMPS_S8) || defined(ARVAE_STAMPS_GRU) || defined(ARVAE_STAMPS_TICK)
#include <hip/hip_runtime.h>

#ifndef GRU_STAMP_WAVE
#define GRU_STAMP_WAVE 0
#endif

namespace arvae {

template <int ROWS_, int SLOTS_, int WORDS_>
struct alignas(16) StampTable {
    static_assert(WORDS_ == 1 || WORDS_ == 2, "a stamp is the wall clock, or {cycle counter, wall clock}");
    static constexpr int ROWS = ROWS_, SLOTS = SLOTS_, WORDS = WORDS_, COUNT = ROWS * SLOTS * WORDS;
    unsigned long long w[COUNT];
};

// ARVAE_STAMP_TABLE(family, rows, slots, words): the table g_<family>_stamps and its reader.  (A kernel file that keeps its
// device symbols in an unnamed namespace declares the two apart: a function declared in there would not be exported.)
#define ARVAE_STAMP_TABLE_ONLY(family, ROWS, SLOTS, WORDS) __device__ ::arvae::StampTable<ROWS, SLOTS, WORDS> g_##family##_stamps;
// the reader copies count words of the table into out; non-zero, and nothing copied, when count exceeds the table
#define ARVAE_STAMP_READER(family)                                                                                           \
    extern "C" int arvae_debug_##family##_stamps(unsigned long long *out, int count) {                                       \
        if (count < 0 || count > decltype(g_##family##_stamps)::COUNT) return -1;                                            \
        return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_##family##_stamps), sizeof(unsigned long long) * count);           \
    }
#define ARVAE_STAMP_TABLE(family, ROWS, SLOTS, WORDS) ARVAE_STAMP_TABLE_ONLY(family, ROWS, SLOTS, WORDS) ARVAE_STAMP_READER(family)

// One stamp: the 100 MHz wall clock, behind the cycle counter where the table keeps both; rows and slots past the table are
// dropped.  A macro, so that the index arithmetic stays in the caller's own types (blockIdx.x is unsigned, a kernel body's
// workgroup number an int) and a stamped kernel compiles to what it did with its private copy of these lines.
#define ARVAE_STAMP(table, row, slot)                                                                                        \
    do {                                                                                                                     \
        typedef decltype(table) T_;                                                                                          \
        if ((row) < T_::ROWS && (slot) < T_::SLOTS) {                                                                        \
            if (T_::WORDS == 2) table.w[((row) * T_::SLOTS + (slot)) * 2] = __builtin_readcyclecounter();                    \
            table.w[((row) * T_::SLOTS + (slot)) * T_::WORDS + T_::WORDS - 1] = wall_clock64();                              \
        }                                                                                                                    \
    } while (0)

// cycles per phase, summed in registers: mark(k) adds the cycles since the last mark (or the construction) to phase k
template <int N>
struct PhaseSums {
    unsigned long long sum[N] = {}, last = __builtin_readcyclecounter();
    __device__ __forceinline__ void mark(int k) {
        const unsigned long long now = __builtin_readcyclecounter();
        sum[k] += now - last;
        last = now;
    }
    // the sums and one more word (the step, tick or tile count they were summed over) into a [1][N + 1][1] table
    __device__ __forceinline__ void flush(StampTable<1, N + 1, 1> &t, unsigned long long extra) const {
        for (int k = 0; k < N; ++k) t.w[k] = sum[k];
        t.w[N] = extra;
    }
};

// a value the phase in front of a stamp must have produced (the compiler keeps its computation on that side of the stamp)
__device__ __forceinline__ void stamp_depend(float v) { asm volatile("" ::"v"(v)); }

// what a family waits for in front of a stamp (none waits for more than it did when it was written)
__device__ __forceinline__ void stamp_wait_all() { __builtin_amdgcn_s_waitcnt(0); }                       // every counter
__device__ __forceinline__ void stamp_wait_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }   // global loads
__device__ __forceinline__ void stamp_wait_lds() { __builtin_amdgcn_s_waitcnt(0xc07f); }                  // lgkmcnt(0): LDS traffic

}  // namespace arvae
#endif
