// test_binary_plan.cpp -- stand-alone check of csrc/hip/binary_plan.h (no device, no HIP): the op-code tables, every refusal, the form
// and vector arm a descriptor takes, the chan form's lane arithmetic, and the bounds next to 2^31.  Built and run under AddressSanitizer and
// UBSan by tests/test_const_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "binary_plan.h"
#include "si_magic.h"

using namespace si_binary_plan;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static SiBinaryDesc Desc(int d0, int d1, int d2, int d3, int stages = 1) {
    SiBinaryDesc d{};
    d.d[0] = d0; d.d[1] = d1; d.d[2] = d2; d.d[3] = d3;
    d.x_ld = d.out_ld = d3;
    d.stages = stages;
    d.op[0] = 2; d.op[1] = 0;
    return d;
}

// dense strides of a constant that has x's extent where mask[i] and is broadcast elsewhere
static void SetConst(SiBinaryDesc& d, int stage, const int (&mask)[4]) {
    int* s = stage == 0 ? d.c0_stride : d.c1_stride;
    int run = 1;
    for (int i = 3; i >= 0; --i) {
        s[i] = mask[i] && d.d[i] > 1 ? run : 0;
        if (mask[i]) run *= d.d[i];
    }
}

int main() {
    const void* const A = reinterpret_cast<const void*>(uintptr_t(1) << 20);        // 16-byte aligned
    const void* const U = reinterpret_cast<const void*>((uintptr_t(1) << 20) + 4);  // not
    Plan p;

    // ---- tables
    const int known[10] = {0, 1, 2, 3, 6, 7, 8, 9, 10, 11};
    for (int op = -3; op < 16; ++op) {
        bool in = false;
        for (int k : known) in = in || k == op;
        CHECK(si_binary_op_known(op) == in);
        if (in) {
            CHECK(si_binary_op_known(si_binary_op_reversed(op)));
            CHECK(si_binary_op_reversed(si_binary_op_reversed(op)) == op);
        }
    }
    CHECK(si_binary_op_reversed(0) == 0 && si_binary_op_reversed(2) == 2 && si_binary_op_reversed(1) == 7 && si_binary_op_reversed(3) == 8 &&
          si_binary_op_reversed(6) == 9 && si_binary_op_reversed(10) == 11);

    // ---- forms: every broadcast mask of one constant over [2,5,7,8]
    for (int m = 0; m < 16; ++m) {
        SiBinaryDesc d = Desc(2, 5, 7, 8);
        const int mask[4] = {(m >> 3) & 1, (m >> 2) & 1, (m >> 1) & 1, m & 1};
        SetConst(d, 0, mask);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0);
        const int want = !(mask[0] || mask[1] || mask[2]) ? kChan : !mask[3] ? kPixel : kFull;
        CHECK(p.form == want);
        CHECK(p.vw == 4 && p.cv == 2 && p.pixels == 70u && p.items == 140u && p.blocks == 1u);
        if (p.form == kChan) CHECK(p.lanes % (unsigned)p.cv == 0 && p.lanes == p.pixel_step * (unsigned)p.cv && p.pixel_step >= 1 && p.pixel_step <= p.pixels);
        CHECK(p.cvec[0] == (mask[3] ? 1 : 0));
        // halves: 8 per lane
        CHECK(MakePlan(&d, A, A, nullptr, A, 2, p) == 0 && p.vw == 8 && p.cv == 1);
    }
    // two stages: the form has to suit both constants
    {
        SiBinaryDesc d = Desc(2, 5, 7, 8, 2);
        const int chan[4] = {0, 0, 0, 1}, pix[4] = {0, 1, 1, 0}, scalar[4] = {0, 0, 0, 0}, all[4] = {1, 1, 1, 1};
        SetConst(d, 0, chan); SetConst(d, 1, chan);
        CHECK(MakePlan(&d, A, A, A, A, 4, p) == 0 && p.form == kChan);
        SetConst(d, 1, scalar);
        CHECK(MakePlan(&d, A, A, A, A, 4, p) == 0 && p.form == kChan);
        SetConst(d, 0, pix);
        CHECK(MakePlan(&d, A, A, A, A, 4, p) == 0 && p.form == kPixel);
        SetConst(d, 1, chan);
        CHECK(MakePlan(&d, A, A, A, A, 4, p) == 0 && p.form == kFull && p.cvec[0] == 0 && p.cvec[1] == 1);
        SetConst(d, 0, all);
        CHECK(MakePlan(&d, A, A, A, A, 4, p) == 0 && p.form == kFull && p.cvec[0] == 1);
        CHECK(MakePlan(&d, A, U, A, A, 4, p) == 0 && p.form == kFull && p.cvec[0] == 0 && p.cvec[1] == 1 && p.vw == 4);   // an unaligned constant alone
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);                                                          // two stages need c1
    }
    // the scalar arm: odd d3, odd strides, unaligned pointers
    {
        SiBinaryDesc d = Desc(1, 3, 5, 7);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.vw == 1 && p.cv == 7 && p.items == 105u);
        d = Desc(1, 3, 5, 8);
        CHECK(MakePlan(&d, U, A, nullptr, A, 4, p) == 0 && p.vw == 1);
        CHECK(MakePlan(&d, A, A, nullptr, U, 4, p) == 0 && p.vw == 1);
        d.x_ld = 9;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.vw == 1);
        d.x_ld = 12; d.out_ld = 16;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.vw == 4);
        CHECK(MakePlan(&d, A, A, nullptr, A, 2, p) == 0 && p.vw == 1);   // 12 halves are not whole 16-byte pieces
    }
    // the grid: capped, and the chan form's lanes a multiple of the run
    {
        SiBinaryDesc d = Desc(4, 64, 64, 96);   // 16384 pixels, 24 pieces per run
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.form == kChan && p.items == 16384u * 24u && p.blocks == (16384u * 24u + 255u) / 256u);
        d = Desc(32, 80, 80, 128);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.blocks == kGridCap && p.lanes == kGridCap * 256u && p.pixel_step == kGridCap * 8u);
        d = Desc(1, 5, 7, 12);
        d.grid_cap = 1;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.blocks == 1u && p.form == kChan && p.cv == 3 && p.pixel_step == 35u && p.lanes == 105u);
        d = Desc(1, 50, 70, 12);
        d.grid_cap = 1;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.blocks == 1u && p.pixel_step == 85u && p.lanes == 255u);   // 256 / 3 runs per pass
        d = Desc(1, 1, 4, 2048);                 // a run longer than one workgroup under a cap of one: no lane could keep its place
        d.grid_cap = 1;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.cv == 512 && p.form == kPixel);
        const int chan[4] = {0, 0, 0, 1};
        SetConst(d, 0, chan);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.form == kFull);
        d.grid_cap = 2;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.form == kChan && p.pixel_step == 1u && p.lanes == 512u);
    }

    // ---- refusals
    {
        SiBinaryDesc d = Desc(2, 5, 7, 8);
        CHECK(MakePlan(nullptr, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        CHECK(MakePlan(&d, nullptr, A, nullptr, A, 4, p) == SI_E_BADARG);
        CHECK(MakePlan(&d, A, nullptr, nullptr, A, 4, p) == SI_E_BADARG);
        CHECK(MakePlan(&d, A, A, nullptr, nullptr, 4, p) == SI_E_BADARG);
        for (int i = 0; i < 4; ++i)
            for (int v : {0, -1}) {
                SiBinaryDesc b = d;
                b.d[i] = v;
                CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
            }
        SiBinaryDesc b = d;
        b.x_ld = 7;
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        b = d; b.out_ld = 7;
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        b = d; b.stages = 0;
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        b = d; b.stages = 3;
        CHECK(MakePlan(&b, A, A, A, A, 4, p) == SI_E_BADARG);
        b = d; b.c0_stride[2] = -1;
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        b = d; b.grid_cap = -1;
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        for (int op : {4, 5, 12, -1}) {
            b = d; b.op[0] = op;
            CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_UNSUPPORTED);
            b = d; b.stages = 2; b.op[1] = op;
            CHECK(MakePlan(&b, A, A, A, A, 4, p) == SI_E_UNSUPPORTED);
        }
        b = d; b.op[1] = 5;                       // the second code is not looked at with one stage
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == 0);
        b = d; b.op[0] = 5; b.d[0] = 0;           // an argument error comes first
        CHECK(MakePlan(&b, A, A, nullptr, A, 4, p) == SI_E_BADARG);
    }

    // ---- next to 2^31: x and out hold pixels * ld elements, a constant its last offset + 1
    {
        SiBinaryDesc d = Desc(1, 1, 1 << 27, 15);            // 2^27 * 15 < 2^31 - 1
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.items == (1u << 27) * 15u && p.blocks == kGridCap);
        d.x_ld = 16;                                         // 2^31
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        d.x_ld = 15; d.out_ld = 16;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        d = Desc(1 << 11, 1 << 10, 1 << 10, 1);              // 2^31 pixels
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        d = Desc(0x7fffffff, 1, 1, 1);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.pixels == 0x7fffffffu);
        d = Desc(0x7fffffff, 0x7fffffff, 0x7fffffff, 1);     // products that overflow 64 bits if they were formed at once
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        d = Desc(0x7fffffff, 2, 1, 1);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        // the constant: strides of 0 keep any extent legal, a stride that carries the last element past the limit does not
        d = Desc(1 << 10, 1 << 10, 1 << 10, 1);
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.form == kChan);
        d.c0_stride[0] = 1 << 20; d.c0_stride[1] = 1 << 10; d.c0_stride[2] = 1;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0 && p.form == kPixel);     // last offset 2^30 - 1
        d.c0_stride[0] = (1 << 21) + 1025;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0);                         // last offset 2^31 - 2: the largest that is accepted
        d.c0_stride[0] = (1 << 21) + 1026;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);               // last offset 2^31 + 1021
        d.c0_stride[0] = 0x7fffffff;
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == SI_E_BADARG);
        d.c0_stride[0] = 0; d.c0_stride[3] = 0x7fffffff;                           // d3 = 1: the stride is never applied
        CHECK(MakePlan(&d, A, A, nullptr, A, 4, p) == 0);
    }

    // ---- the kernel's index decomposition: si_fast_divmod is si_fast_div with the remainder, over the contract's corners
    for (int d : {1, 2, 3, 7, 8, 105, 257, 65535, 0x7fffffff}) {
        const unsigned mg = si_magic(d);
        for (int n : {0, 1, d - 1, d, d < 0x7fffffff ? d + 1 : d, 12345, 0x7ffffffe, 0x7fffffff}) {
            if (n < 0) continue;
            int rem = -1;
            const int q = si_fast_divmod(n, d, mg, rem);
            CHECK(q == n / d && rem == n % d && q == si_fast_div(n, d, mg));
        }
    }

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("binary plan ok\n");
    return 0;
}
