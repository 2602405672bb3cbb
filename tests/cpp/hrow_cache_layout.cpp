// hrow_cache_layout.cpp — host program of tests/test_hrow_cache_layout.py: the layout of the h rows' cache
// region (Cfg::HROW_CACHE) in a workgroup's slot of the global workspace, from the constants of
// csrc/mpcg_sqp.h.  One line per instance:
//   <name> cache <HROW_CACHE> r0 <first cached h slot> slots <n> vals <n> region <doubles> offset <doubles>
//   slot <doubles> ws <bytes per solve> ws_without <bytes per solve without the region> onto <0|1> rows <0|1>
// onto: (slot, value, lane) -> hrow_idx is one to one onto [0, region); rows: every ellipsoid row of every part
// lies in a cached slot and (HROW_CACHE 1) every cached slot holds one on some part.
#include <cstdio>
#include <vector>

#include "mpcg_sqp.h"

using namespace mpcg;

template <class C>
void report(const char* name) {
    bool onto = true, rows = true;
    std::vector<int> hit(C::HROW_DOUBLES, 0);
    for (int s = 0; s < C::HROW_SLOTS; ++s)
        for (int v = 0; v < C::HROW_VALS; ++v)
            for (int l = 0; l < 64; ++l) {
                const int i = C::hrow_idx(s, v, l);
                if (i < 0 || i >= C::HROW_DOUBLES) onto = false;
                else ++hit[i];
                // a value's 64 lanes are contiguous: one coalesced access per wave
                if (l > 0 && i != C::hrow_idx(s, v, l - 1) + 1) onto = false;
            }
    for (int h : hit) onto = onto && h == 1;
    if (C::HROW_CACHE > 0) {
        std::vector<int> used(C::HROW_SLOTS, 0);
        for (int part = 0; part < C::PARTS; ++part)
            for (int r = 0; r < C::HS; ++r) {
                const int hh = part + C::PARTS * r;
                if (hh < C::NL || hh >= C::NL + C::NE) continue;
                if (r < C::HROW_R0 || r >= C::HROW_R0 + C::HROW_SLOTS) rows = false;
                else used[r - C::HROW_R0] = 1;
            }
        if (C::HROW_CACHE == 1)
            for (int u : used) rows = rows && u == 1;
    }
    const size_t tail = tail_levels<C>() ? tail::WORDS_PER_SOLVE / 2 + carry_doubles<C>() : 0;
    printf("%s cache %d r0 %d slots %d vals %d region %d offset %zu slot %zu ws %zu ws_without %zu onto %d rows %d\n",
           name, (int)C::HROW_CACHE, C::HROW_R0, C::HROW_SLOTS, C::HROW_VALS, C::HROW_DOUBLES, hrow_offset<C>(),
           slot_doubles<C>(), ws_doubles<C>() * sizeof(double),
           (gfh_doubles<C>() + itref_doubles<C>() + tail) * sizeof(double), (int)onto, (int)rows);
}

int main() {
    report<Cfg<20, 4, 4, 0, 5, 0>>("C1");
    report<Cfg<20, 8, 8, 0, 5, 0>>("C2");
    report<Cfg<10, 2, 2, 0, 5, 0>>("T10");
    report<Cfg<30, 12, 12, 0, 5, 0>>("C4");
    report<Cfg<20, 0, 0, 24, 6, 0>>("C5");
    report<Cfg<30, 4, 4, 0, 5, 0>>("JS");
    report<Cfg<30, 5, 5, 0, 5, 0>>("JD");
    report<Cfg<30, 0, 0, 12, 6, 1>>("C3");
    report<Cfg<25, 3, 3, 0, 5, 0>>("G25");
    return 0;
}
