// pt_render_kernels.h -- every k_render_sm instantiation the library builds, one line each, by the
// template's arguments: X(COUNT, LDS, MINW, MULTI, SPLIT, PADN, NT, WIDE).  pt_render.hip expands the list
// into its {key, kernel} table; kernel_key (pt_launch_plan.cpp) makes the key a launch uses, and
// tests/test_launch_plan.py checks on the CPU that every key it makes is a line here.
#pragma once

// clang-format off
#define PT_RENDER_KERNELS(X)                                                                   \
    /* counting builds: the binary walks, 5 waves per SIMD */                                  \
    X(true,  true,  5, false, false, false, 256, false)                                        \
    X(true,  true,  5, false, true,  false, 256, false)                                        \
    X(true,  true,  5, true,  false, false, 256, false)                                        \
    X(true,  true,  5, true,  true,  false, 256, false)                                        \
    X(true,  false, 5, false, false, false, 256, false)                                        \
    X(true,  false, 5, false, true,  false, 256, false)                                        \
    X(true,  false, 5, true,  false, false, 256, false)                                        \
    X(true,  false, 5, true,  true,  false, 256, false)                                        \
    /* scene in LDS, 256 threads */                                                            \
    X(false, true,  5, false, false, false, 256, false)                                        \
    X(false, true,  5, false, true,  false, 256, false)                                        \
    X(false, true,  5, true,  false, false, 256, false)                                        \
    X(false, true,  5, true,  true,  false, 256, false)                                        \
    X(false, true,  6, false, false, false, 256, false)                                        \
    X(false, true,  6, false, true,  false, 256, false)                                        \
    X(false, true,  6, true,  false, false, 256, false)                                        \
    X(false, true,  6, true,  true,  false, 256, false)                                        \
    X(false, true,  7, false, true,  false, 256, false)                                        \
    X(false, true,  7, false, true,  true,  256, false)                                        \
    X(false, true,  8, false, true,  false, 256, false)                                        \
    /* scene in LDS, one copy shared by a wide workgroup */                                    \
    X(false, true,  6, false, false, false, 512, false)                                        \
    X(false, true,  6, false, true,  false, 512, false)                                        \
    X(false, true,  6, false, false, false, 768, false)                                        \
    X(false, true,  6, false, true,  false, 768, false)                                        \
    X(false, true,  4, false, false, false, 1024, false)                                       \
    X(false, true,  4, false, true,  false, 1024, false)                                       \
    /* scene in global memory, binary walk */                                                  \
    X(false, false, 5, false, false, false, 256, false)                                        \
    X(false, false, 5, false, true,  false, 256, false)                                        \
    X(false, false, 5, true,  false, false, 256, false)                                        \
    X(false, false, 5, true,  true,  false, 256, false)                                        \
    X(false, false, 6, false, false, false, 256, false)                                        \
    X(false, false, 6, false, true,  false, 256, false)                                        \
    X(false, false, 6, true,  false, false, 256, false)                                        \
    X(false, false, 6, true,  true,  false, 256, false)                                        \
    X(false, false, 7, false, true,  false, 256, false)                                        \
    X(false, false, 8, false, true,  false, 256, false)                                        \
    /* scene in global memory, wide walk */                                                    \
    X(false, false, 5, false, false, false, 256, true)                                         \
    X(false, false, 5, false, true,  false, 256, true)                                         \
    X(false, false, 6, false, false, false, 256, true)                                         \
    X(false, false, 6, false, true,  false, 256, true)                                         \
    X(false, false, 6, true,  false, false, 256, true)                                         \
    X(false, false, 6, true,  true,  false, 256, true)                                         \
    X(false, false, 7, false, false, false, 256, true)                                         \
    X(false, false, 7, false, true,  false, 256, true)                                         \
    X(false, false, 6, false, false, false, 512, true)                                         \
    X(false, false, 6, false, true,  false, 512, true)                                         \
    X(false, false, 6, false, false, false, 768, true)                                         \
    X(false, false, 6, false, true,  false, 768, true)                                         \
    X(false, false, 4, false, false, false, 1024, true)                                        \
    X(false, false, 4, false, true,  false, 1024, true)
// The lines also built with the template's last argument, COMMON: the default configuration's launch-uniform facts as
// constants (pt_render.hip, LaunchFacts).  A launch runs one when its plan says `common` and enqueue_render finds the
// remaining facts true; its generic line above stays the fall-back.
#define PT_RENDER_KERNELS_COMMON(X)                                                            \
    X(false, true,  7, false, true,  true,  256, false)
// clang-format on
