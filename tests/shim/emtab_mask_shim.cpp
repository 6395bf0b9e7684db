// Host build of the record consumer's bit masks (cnf2_emtab.h: keep_if_bit, emtab_part_rec) for tests/test_emtab_mask_host.py,
// which restates the select form itself and compares bit patterns.
#include <stdint.h>
#include <string.h>

#include "cnf2_window.h"
#include "cnf2_emtab.h"

using namespace cnf2;

// the bits of keep_if_bit(bits, e, v) for the double whose bits are vbits
extern "C" uint64_t shim_keep_if_bit(uint32_t bits, int e, uint64_t vbits)
{
    double v;
    memcpy(&v, &vbits, sizeof(v));
    const double r = keep_if_bit(bits, e, v);
    uint64_t     u;
    memcpy(&u, &r, sizeof(u));
    return u;
}

// emtab_part_rec<classes, packed> of part (P, f) for n records that differ in `bits` only.  root5 = a0, a1, s0, s1, hw; rec6 = Bp,
// Cp, Kp, t0, t1, oo.  out [n][3][8]: the bits of entry e of table kind; an entry that is not handed over keeps `unset`.
// cw [n][2]: the root weights' bits.
extern "C" void shim_part_rec(int classes, int packed, int P, int f, const double* root5, const double* rec6, const uint32_t* bits,
                              int n, uint64_t unset, uint64_t* out, uint64_t* cw)
{
    Slot root;
    root.a0 = (int)root5[0];
    root.a1 = (int)root5[1];
    root.s0 = root5[2];
    root.s1 = root5[3];
    root.hw = root5[4];
    for (int i = 0; i < n; i++) {
        LineRec r;
        r.Bp = rec6[0];
        r.Cp = rec6[1];
        r.Kp = rec6[2];
        r.t0 = rec6[3];
        r.t1 = rec6[4];
        r.oo = rec6[5];
        r.bits = bits[i];
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        uint64_t* o = out + (size_t)i * 24;
        for (int k = 0; k < 24; k++) o[k] = unset;
        double cwv[2];
        auto   put = [&](int kind, int e, double v) { memcpy(&o[kind * 8 + e], &v, sizeof(v)); };
        if (classes && packed) emtab_part_rec<true, true>(P, f, root, r, put, cwv);
        else if (classes) emtab_part_rec<true, false>(P, f, root, r, put, cwv);
        else if (packed) emtab_part_rec<false, true>(P, f, root, r, put, cwv);
        else emtab_part_rec<false, false>(P, f, root, r, put, cwv);
        memcpy(cw + (size_t)i * 2, cwv, sizeof(cwv));
    }
}
