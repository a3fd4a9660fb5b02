// Conv2d's host-side decisions on their own, without a device: for a table of layers set up through the public fields, which kernel family
// serves an (input, output) storage pair (the route), which packed weight image that family reads, and the Winograd tile.  The expected values
// are spelled out here, row by row; they were recorded from the layer as it stood before the route / image enums existed (its PrecisionMode and
// WinogradTile), so a change of any row is a change of which kernel a network runs.  KernelName() is not covered: it needs bound tensor nodes.
// Stand-alone; built against the two product libraries by tests/test_conv_route_cpu.py.
#include <cstdio>
#include <cstring>

#include "layer/conv_2d.h"
#include "tensor_node.h"

using SimpleInfer::Conv2d;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

// the codes of Conv2d::Route and of the weight image, by value: not read from the header
enum { rIgemmF32 = 0, rWino23F32, rWino43F32, rIgemmF16, rStemF16, rDepthwiseF16, rSplit3, rWinoSplit, rStemSplit };
enum { iNone = 0, iIgemmF32, iWino23F32, iWino43F32, iIgemmF16, iStemF16, iSplit3, iWino23Split, iStemSplit3 };
enum { aAuto = 0, aIgemm, aWino23, aWino43 };

struct Spec {
    const char* name;
    int ic, oc, k, s, p, d, g;
    int algo;
    bool prefer43;
    int sibling_oc;   // 0: none; else a fused 1x1 sibling with this many output channels
    bool residual;
};

static const Spec kLayers[] = {
    /*  0 */ {"stem 3->32 6x6 s2 p2", 3, 32, 6, 2, 2, 1, 1, aAuto, false, 0, false},
    /*  1 */ {"stem 3->64 7x7 s2 p3", 3, 64, 7, 2, 3, 1, 1, aAuto, false, 0, false},
    /*  2 */ {"32->32 3x3 s1 p1", 32, 32, 3, 1, 1, 1, 1, aAuto, false, 0, false},
    /*  3 */ {"16->32 3x3 s1 p1", 16, 32, 3, 1, 1, 1, 1, aAuto, false, 0, false},
    /*  4 */ {"64->64 3x3 s1 auto", 64, 64, 3, 1, 1, 1, 1, aAuto, false, 0, false},
    /*  5 */ {"64->64 3x3 s1 igemm", 64, 64, 3, 1, 1, 1, 1, aIgemm, false, 0, false},
    /*  6 */ {"64->64 3x3 s1 wino23", 64, 64, 3, 1, 1, 1, 1, aWino23, false, 0, false},
    /*  7 */ {"64->64 3x3 s1 wino43", 64, 64, 3, 1, 1, 1, 1, aWino43, false, 0, false},
    /*  8 */ {"64->64 3x3 s1 auto, prefer F(4,3)", 64, 64, 3, 1, 1, 1, 1, aAuto, true, 0, false},
    /*  9 */ {"32->64 3x3 s2 p1", 32, 64, 3, 2, 1, 1, 1, aAuto, false, 0, false},
    /* 10 */ {"128->128 3x3 s2 p1", 128, 128, 3, 2, 1, 1, 1, aAuto, false, 0, false},
    /* 11 */ {"512->256 1x1", 512, 256, 1, 1, 0, 1, 1, aAuto, false, 0, false},
    /* 12 */ {"128->128 1x1", 128, 128, 1, 1, 0, 1, 1, aAuto, false, 0, false},
    /* 13 */ {"depthwise 32 3x3", 32, 32, 3, 1, 1, 1, 32, aAuto, false, 0, false},
    /* 14 */ {"depthwise 12 3x3", 12, 12, 3, 1, 1, 1, 12, aAuto, false, 0, false},
    /* 15 */ {"64->64 3x3 groups 2", 64, 64, 3, 1, 1, 1, 2, aAuto, false, 0, false},
    /* 16 */ {"64->64 3x3 dilation 2", 64, 64, 3, 1, 2, 2, 1, aAuto, false, 0, false},
    /* 17 */ {"64->32 | 32 1x1 siblings", 64, 32, 1, 1, 0, 1, 1, aAuto, false, 32, false},
    /* 18 */ {"64->64 3x3 s1 + residual", 64, 64, 3, 1, 1, 1, 1, aAuto, false, 0, true},
    /* 19 */ {"stem 3->32 6x6 s2 + residual", 3, 32, 6, 2, 2, 1, 1, aAuto, false, 0, true},
    /* 20 */ {"256->128 | 128 1x1 siblings", 256, 128, 1, 1, 0, 1, 1, aAuto, false, 128, false},
    /* 21 */ {"256->256 3x3 s1 auto", 256, 256, 3, 1, 1, 1, 1, aAuto, false, 0, false},
    /* 22 */ {"Detect 128->255 1x1", 128, 255, 1, 1, 0, 1, 1, aAuto, false, 0, false},
    /* 23 */ {"Detect 64->255 1x1", 64, 255, 1, 1, 0, 1, 1, aAuto, false, 0, false},
};
static const int kNumLayers = sizeof(kLayers) / sizeof(kLayers[0]);

// engine option f32_split: off, on at policy 1..4, and on at policy 4 then demoted (DemoteSplit: what a range trip or a refused view does)
enum Opt { kOff = 0, kL1, kL2, kL3, kL4, kDemoted, kNumOpts };
static const char* const kOptNames[] = {"off", "split L1", "split L2", "split L3", "split L4", "demoted"};

struct Want { int route, image, tile; };
struct Row {
    int layer;
    Opt opt;
    Want pair[3];   // fp32 -> fp32, half -> half, fp32 -> half
};
// the Detect-head entry point (ForwardYolo) makes a choice of its own, from the input's storage type alone: fp32 input, half input
struct YoloRow {
    int layer;
    Opt opt;
    Want in[2];
};
static const int kYoloLayers[] = {22, 23};
static const bool kPairs[3][2] = {{false, false}, {true, true}, {false, true}};
static const char* const kPairNames[] = {"f32->f32", "f16->f16", "f32->f16"};

static const Row kRows[] = {
    // 0: stem 3->32 6x6 s2 p2
    {0, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {0, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {0, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {0, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {0, kL4, {{rStemSplit, iStemSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {0, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    // 1: stem 3->64 7x7 s2 p3
    {1, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {1, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {1, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {1, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {1, kL4, {{rStemSplit, iStemSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    {1, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rStemF16, iStemF16, 0}}},
    // 2: 32->32 3x3 s1 p1
    {2, kOff, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {2, kL1, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {2, kL2, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {2, kL3, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {2, kL4, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {2, kDemoted, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 3: 16->32 3x3 s1 p1
    {3, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {3, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {3, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {3, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {3, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {3, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 4: 64->64 3x3 s1 auto
    {4, kOff, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {4, kL1, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {4, kL2, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {4, kL3, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {4, kL4, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {4, kDemoted, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 5: 64->64 3x3 s1 igemm
    {5, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {5, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {5, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {5, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {5, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {5, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 6: 64->64 3x3 s1 wino23
    {6, kOff, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {6, kL1, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {6, kL2, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {6, kL3, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {6, kL4, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {6, kDemoted, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 7: 64->64 3x3 s1 wino43
    {7, kOff, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {7, kL1, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {7, kL2, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {7, kL3, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {7, kL4, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {7, kDemoted, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 8: 64->64 3x3 s1 auto, prefer F(4,3)
    {8, kOff, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {8, kL1, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {8, kL2, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {8, kL3, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {8, kL4, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {8, kDemoted, {{rWino43F32, iWino43F32, 4}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 9: 32->64 3x3 s2 p1
    {9, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {9, kL1, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {9, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {9, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {9, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {9, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 10: 128->128 3x3 s2 p1
    {10, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {10, kL1, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {10, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {10, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {10, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {10, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 11: 512->256 1x1
    {11, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {11, kL1, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {11, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {11, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {11, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {11, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 12: 128->128 1x1
    {12, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {12, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {12, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {12, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {12, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {12, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 13: depthwise 32 3x3
    {13, kOff, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {13, kL1, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {13, kL2, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {13, kL3, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {13, kL4, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {13, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 14: depthwise 12 3x3
    {14, kOff, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {14, kL1, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {14, kL2, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {14, kL3, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {14, kL4, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {14, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rDepthwiseF16, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 15: 64->64 3x3 groups 2
    {15, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {15, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {15, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {15, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {15, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {15, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 16: 64->64 3x3 dilation 2
    {16, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {16, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {16, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {16, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {16, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {16, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 17: 64->32 | 32 1x1 siblings
    {17, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {17, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {17, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {17, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {17, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {17, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 18: 64->64 3x3 s1 + residual
    {18, kOff, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {18, kL1, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {18, kL2, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {18, kL3, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {18, kL4, {{rWinoSplit, iWino23Split, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {18, kDemoted, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 19: stem 3->32 6x6 s2 + residual
    {19, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {19, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {19, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {19, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {19, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {19, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 20: 256->128 | 128 1x1 siblings
    {20, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {20, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {20, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {20, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {20, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {20, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 21: 256->256 3x3 s1 auto
    {21, kOff, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {21, kL1, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {21, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {21, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {21, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {21, kDemoted, {{rWino23F32, iWino23F32, 2}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 22: Detect 128->255 1x1
    {22, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 23: Detect 64->255 1x1
    {23, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}, {rIgemmF16, iIgemmF16, 0}}},
};
static const int kNumRows = sizeof(kRows) / sizeof(kRows[0]);

static const YoloRow kYoloRows[] = {
    // 22: Detect 128->255 1x1
    {22, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL1, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL2, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL3, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kL4, {{rSplit3, iSplit3, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {22, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    // 23: Detect 64->255 1x1
    {23, kOff, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL1, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL2, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL3, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kL4, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
    {23, kDemoted, {{rIgemmF32, iIgemmF32, 0}, {rIgemmF16, iIgemmF16, 0}}},
};
static const int kNumYoloRows = sizeof(kYoloRows) / sizeof(kYoloRows[0]);

struct Built {
    Conv2d conv, sibling;
    SimpleInfer::TensorNode residual;
};

static void Build(const Spec& s, Opt opt, Built& b) {
    auto set = [](Conv2d& c, int ic, int oc, int k, int st, int p, int d, int g) {
        c.in_channels_ = ic; c.out_channels_ = oc; c.groups_ = g;
        c.kernel_h_ = c.kernel_w_ = k; c.stride_h_ = c.stride_w_ = st; c.dilation_h_ = c.dilation_w_ = d;
        c.padding_t_ = c.padding_b_ = c.padding_l_ = c.padding_r_ = p;
    };
    set(b.conv, s.ic, s.oc, s.k, s.s, s.p, s.d, s.g);
    b.conv.algo_ = static_cast<Conv2d::Algo>(s.algo);
    b.conv.prefer_wino43_ = s.prefer43;
    if (s.sibling_oc) {
        set(b.sibling, s.ic, s.sibling_oc, 1, 1, 0, 1, 1);
        b.conv.sibling_ = &b.sibling;
    }
    if (s.residual) b.conv.residual_node_ = &b.residual;
    if (opt != kOff) {
        b.conv.f32_split_ = true;
        b.conv.f32_split_level_ = opt == kDemoted ? 4 : (int)opt;
    }
    if (opt == kDemoted) b.conv.DemoteSplit();
}

// --- ask begin: the only lines that name the accessors
static Want Ask(const Conv2d& c, bool in_half, bool out_half) {
    const Conv2d::RouteInfo r = c.DescribeRoute(in_half, out_half);
    return {r.route, r.image, r.wino_tile};
}
static Want AskYolo(const Conv2d& c, bool in_half) {
    const Conv2d::RouteInfo r = c.DescribeYoloRoute(in_half);
    return {r.route, r.image, r.wino_tile};
}
// --- ask end

static void Compare(int layer, Opt opt, const char* what, const Want& got, const Want& want) {
    if (got.route == want.route && got.image == want.image && got.tile == want.tile) return;
    std::printf("[%s] %s, %s: route %d image %d tile %d, expected route %d image %d tile %d\n", kLayers[layer].name, kOptNames[opt], what,
                got.route, got.image, got.tile, want.route, want.image, want.tile);
    ++failures;
}

int main() {
    // one row per (layer, option), in order: none missing, none twice
    EXPECT(kNumRows == kNumLayers * (int)kNumOpts);
    for (int i = 0; i < kNumRows; ++i) {
        const Row& row = kRows[i];
        EXPECT(row.layer == i / (int)kNumOpts && (int)row.opt == i % (int)kNumOpts);
        if (row.layer < 0 || row.layer >= kNumLayers) continue;
        Built b;
        Build(kLayers[row.layer], row.opt, b);
        for (int p = 0; p < 3; ++p) Compare(row.layer, row.opt, kPairNames[p], Ask(b.conv, kPairs[p][0], kPairs[p][1]), row.pair[p]);
        // asking changes nothing: the two fields the launch reads are still what the constructor left
        EXPECT(!b.conv.use_winograd_ && b.conv.wino_tile_ == 0);
    }
    EXPECT(kNumYoloRows == 2 * (int)kNumOpts);
    for (int i = 0; i < kNumYoloRows; ++i) {
        const YoloRow& row = kYoloRows[i];
        EXPECT(row.layer == kYoloLayers[i / (int)kNumOpts] && (int)row.opt == i % (int)kNumOpts);
        if (row.layer < 0 || row.layer >= kNumLayers) continue;
        Built b;
        Build(kLayers[row.layer], row.opt, b);
        Compare(row.layer, row.opt, "yolo, f32 in", AskYolo(b.conv, false), row.in[0]);
        Compare(row.layer, row.opt, "yolo, f16 in", AskYolo(b.conv, true), row.in[1]);
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("conv route ok (%d + %d rows)\n", kNumRows, kNumYoloRows);
    return 0;
}
