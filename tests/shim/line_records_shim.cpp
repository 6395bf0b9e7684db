// Host build of the line records (cnf2_emtab.h: line_record_make, emtab_part_rec) for tests/test_line_records_host.py:
// records + consumer against the general tile producer emtab_part<CLASSES>, bit for bit, over a grid of uniform lines.
#include <stdint.h>
#include <string.h>

#include "cnf2_window.h"
#include "cnf2_emtab.h"
#include "cnf2_lane.h"

using namespace cnf2;

namespace {
const int    ALLELES[5] = {0, 1, 2, 3, 9};
const double SURES[5]   = {0.0, 0.02, 0.37, 0.5, 1.0};
const double HWS[4]     = {0.0, 0.31, 0.5, 1.0};

struct Lcg {
    uint64_t s;
    unsigned next(unsigned n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)((s >> 33) % n);
    }
};

// (a homozygous slot with equal sure: its phase weights are 0 and 1 whatever its haploweight, which therefore varies too)
Slot hom_slot(int ia, int is, int ihw)
{
    Slot d;
    d.a0 = d.a1 = ALLELES[ia];
    d.s0 = d.s1 = SURES[is];
    d.hw = HWS[ihw & 3];
    return d;
}
bool same_bits(const double* a, const double* b, int n) { return memcmp(a, b, sizeof(double) * n) == 0; }
}  // namespace

// Every homozygous (parent, traced, other) triple over the allele and sure grids x every combination of SLOT_RESTRICT0 on the
// three x the 8 parts x `roots` random roots (any two alleles, any two sures, any haploweight).  counts[0] = configurations,
// counts[1] = those whose tables or root weights differ from emtab_part<CLASSES>, counts[2] = those where an entry is neither
// 0 nor the bits of the part's one value, counts[3] = configurations with a nonzero restricted or class-2 entry (the grid
// reaches them).  first_bad[10]: (ip, it, io, restrict mask, part, root a0, a1, is0, is1, ihw) of the first difference.
extern "C" void shim_line_records_grid(int classes, int roots, uint64_t seed, int64_t* counts, int32_t* first_bad)
{
    Lcg rng{seed};
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int ip = 0; ip < 25; ip++)
        for (int it = 0; it < 25; it++)
            for (int io = 0; io < 25; io++) {
                const Slot par = hom_slot(ip / 5, ip % 5, ip + it), trs = hom_slot(it / 5, it % 5, it + io + 1),
                           ots = hom_slot(io / 5, io % 5, io + ip + 2);
                for (int rm = 0; rm < 8; rm++)
                    for (int part = 0; part < 8; part++)
                        for (int k = 0; k < roots; k++) {
                            int   ra[5];
                            for (int j = 0; j < 5; j++) ra[j] = (int)rng.next(j < 4 ? 5 : 4);
                            Slot root;
                            root.a0 = ALLELES[ra[0]];
                            root.a1 = ALLELES[ra[1]];
                            root.s0 = SURES[ra[2]];
                            root.s1 = SURES[ra[3]];
                            root.hw = HWS[ra[4]];
                            PartCfg c;
                            c.P          = part >> 2;
                            c.f          = (part >> 1) & 1;
                            c.firstpar   = part & 1;
                            c.root_attop = false;
                            c.par = SLOT_PRESENT | SLOT_HOM | ((rm & 1) ? SLOT_RESTRICT0 : 0);
                            c.tr  = SLOT_PRESENT | SLOT_HOM | ((rm & 2) ? SLOT_RESTRICT0 : 0);
                            c.ot  = SLOT_PRESENT | SLOT_HOM | ((rm & 4) ? SLOT_RESTRICT0 : 0);
                            double want[3][8] = {}, got[3][8] = {}, cw[2], cw2[2];
                            if (classes) emtab_part<true>(c, root, par, trs, ots, want[0], want[1], want[2], cw);
                            else emtab_part<false>(c, root, par, trs, ots, want[0], want[1], want[2], cw);
                            const int v = c.P ? (c.f ? root.a0 : root.a1) : (c.f ? root.a1 : root.a0);
                            LineRec rec;
                            line_record_make(c.par, c.tr, c.ot, c.firstpar, v, par, trs, ots, &rec);
                            auto out = [&](int kind, int e, double x) { got[kind][e] = x; };
                            if (classes) emtab_part_rec<true>(c.P, c.f, root, rec, out, cw2);
                            else emtab_part_rec<false>(c.P, c.f, root, rec, out, cw2);
                            counts[0]++;
                            const bool ok = same_bits(want[0], got[0], 24) && same_bits(cw, cw2, 2);
                            bool one = true, any = false;
                            for (int kind = 0; kind < 3; kind++)
                                for (int e = 0; e < 8; e++) {
                                    if (want[kind][e] != 0.0 && !same_bits(&want[kind][e], &want[0][0], 1)) one = false;
                                    if (kind > 0 && want[kind][e] != 0.0) any = true;
                                }
                            if (any) counts[3]++;
                            if (!one) counts[2]++;
                            if (!ok) {
                                if (counts[1] == 0) {
                                    const int32_t fb[10] = {ip, it, io, rm, part, root.a0, root.a1, ra[2], ra[3], ra[4]};
                                    memcpy(first_bad, fb, sizeof(fb));
                                }
                                counts[1]++;
                            }
                        }
            }
}
