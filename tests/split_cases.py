"""Case tables and the bar of the float64 accuracy tests of the split-operand MFMA kernels (ar-vae_amd/csrc/splitmath.h), shared by the GPU test
(test_split_kernels_float64.py) and by the CPU model that proves the bar discriminates (test_three_term_arithmetic.py).
No test in here: the tables only.

The bar, for every output tensor:   e_hip <= R * e_cpu + FLOOR
  e_hip   relative L2 distance of the HIP result to the float64 result
  e_cpu   relative L2 distance of torch's fp32 CPU result on the same fp32 inputs to the float64 result
  FLOOR   1e-7: one rounding of an exact result to fp32 is already ~3.4e-8 relative L2, and torch sometimes lands near it
  R       4: the smallest whole number for which the CPU model's separation holds at every reduction length below -- at
          K = 6144 (the longest, the rows-GEMM weight gradient) a sequential fp32 multiply-add chain sits at about 3.7-3.95 x torch's
          error (torch's own figure depends on its BLAS blocking; there the FLOOR term carries part of the margin) and the least
          harmful missing product at about 6.5-7 x; at K = 1024 the two are about 2 x and 8.5 x."""

R = 4.0
FLOOR = 1.0e-7

# ---- stride-1 4x4 links: (hi size, hi channels, lo size, lo channels, pad); lo = hi + 2 pad - 3
CONV_LINKS = {
    'c64_25':     (25, 64, 22, 64, 0),     # Morpho-MNIST 64 -> 64
    'c64to8_22':  (22, 64, 19, 8, 0),      # 64 -> 8
    'c64to16_21': (21, 64, 18, 16, 0),     # a narrow multiple-of-4 output
    'c64_12p1':   (12, 64, 11, 64, 1),     # padded: source rows above / below the image
    'c64to8_9p2': (9, 64, 10, 8, 2),
    'c8to64_22':  (22, 8, 19, 64, 0),      # the mirrored links: the 64-channel side is lo, so link_up is the row-staged one
    'c16to64_21': (21, 16, 18, 64, 0),
    'c8to64_9p2': (9, 8, 10, 64, 2),
}
CONV_BATCHES = (3, 47, 70)                 # fewer and more row-group tiles than CUs

# weight / bias gradients: (link, n).  The reduction runs over n * lo * lo pixels.  The CPU model separates a correct fp32
# accumulation from a missing product only up to a few thousand terms (at 33 880, n = 70 of the 22 x 22 layer, the sequential
# chain's own error has passed the missing product's), so every n here keeps n * lo * lo <= 6144.  That leaves out the batches
# at which the paired-rows kernel gives a workgroup several images (n >= 384): the whole-step tests cover those.
WGRAD_ONLY_LINKS = {'c64_31': (31, 64, 28, 64, 0), 'c64_k3': (14, 64, 12, 64, 0)}     # the second one with 3 x 3 taps
WGRAD_CASES = [('c64_25', 1), ('c64_25', 5), ('c64_25', 12), ('c64to8_22', 1), ('c64to8_22', 7), ('c64to8_22', 17),
               ('c8to64_22', 1), ('c8to64_22', 7), ('c8to64_22', 17),
               ('c64_31', 1), ('c64_31', 7),          # lo wider than 24: conv_wgrad_rows_x3_kernel
               ('c64_k3', 1), ('c64_k3', 11)]         # 3 x 3 taps: conv_wgrad_x3_kernel

# ---- Linear layers: (rows, fin, fout, in_perm, out_perm)
DENSE_WIDE = [(rows, 2888, 256, (8, 361), (0, 0)) for rows in (5, 64, 1024, 1100)] + \
             [(rows, 256, 2888, (0, 0), (8, 361)) for rows in (5, 64, 1024, 1100)]
DENSE_LONG = [(6144, 128, 384, (0, 0), (0, 0)), (2050, 138, 384, (0, 0), (0, 0)), (2311, 10, 384, (0, 0), (0, 0)),
              (6144, 128, 35, (0, 0), (0, 0)), (2048, 256, 130, (0, 0), (0, 0))]
DENSE_SMALL = [(5, 10, 256, (0, 0), (0, 0)), (33, 256, 10, (0, 0), (0, 0)), (8, 256, 512, (0, 0), (0, 0)),
               (64, 512, 256, (0, 0), (0, 0))]


def link_geometry(name):
    """(hi size, hi channels, lo size, lo channels, pad, kernel size) of a named link"""
    return (CONV_LINKS.get(name) or WGRAD_ONLY_LINKS[name]) + (3 if name == 'c64_k3' else 4,)


def reduction_lengths():
    """every reduction length a PRODUCT of the GPU table runs over (the bias sums, plain additions over up to n * hi * hi = 7500
    values, involve no split operand and are outside the separation claim)"""
    ks = set()
    for hi, chi, lo, clo, _pad in CONV_LINKS.values():
        ks.update((16 * chi, 16 * clo))                                  # link_down, link_up
    for name, n in WGRAD_CASES:
        ks.add(n * link_geometry(name)[2] ** 2)                            # pixels
    for rows, fin, fout, _ip, _op in DENSE_WIDE + DENSE_LONG + DENSE_SMALL:
        ks.update((fin, fout, rows))                                     # forward, data gradient, weight gradient
    return sorted(ks)
