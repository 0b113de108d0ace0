// StageLayout (csrc/ssf_stage_layout.hpp) on the CPU: where the host arrays of a call sit in the staging buffer.  Built with
// -fsanitize=address,undefined by tests/test_stage_layout.py.  For every case: each offset is a multiple of 256, the items do
// not overlap, the total is the sum of the aligned sizes of the items that have a host array, and an item without one gets a null
// pointer.
#include <cstddef>
#include <cstdio>
#include <vector>
#include "../../supersurfel_fusion_amd/csrc/ssf_stage_layout.hpp"

static int failures = 0;
#define EXPECT(cond)                                                                      \
    do {                                                                                  \
        if (!(cond)) { std::printf("%s: line %d: %s\n", what, __LINE__, #cond); failures++; } \
    } while (0)

struct Decl { bool present; size_t bytes; };

static void check(const char* what, const std::vector<Decl>& decl) {
    static const char host_byte = 0;                        // any non-null address: the layout never reads through it
    size_t room = 0;                                        // the restatement's total: what a caller would allocate, and no more
    for (const Decl& d : decl) room += d.present ? (d.bytes + 255) / 256 * 256 : 0;
    std::vector<unsigned char> buf(room);
    ssf::StageLayout lay;
    for (size_t i = 0; i < decl.size(); i++) EXPECT(lay.add(decl[i].present ? &host_byte : nullptr, decl[i].bytes) == (int)i);
    EXPECT(lay.n == (int)decl.size());
    size_t sum = 0, end_prev = 0;
    for (size_t i = 0; i < decl.size(); i++) {
        unsigned char* p = lay.at(buf.data(), (int)i);
        if (!decl[i].present) { EXPECT(p == nullptr); continue; }
        EXPECT(p != nullptr);
        if (!p) continue;
        const size_t off = (size_t)(p - buf.data());
        EXPECT(off % 256 == 0);
        EXPECT(off == sum);                                 // the restatement: the aligned sizes of the present items before it
        EXPECT(off >= end_prev);                            // behind everything before it (the items come in order)
        EXPECT(off + decl[i].bytes <= lay.total);
        EXPECT(off + decl[i].bytes <= buf.size());
        p[0] = (unsigned char)i; if (decl[i].bytes) p[decl[i].bytes - 1] = (unsigned char)i;   // (the sanitizer watches the ends)
        end_prev = off + decl[i].bytes;
        sum += (decl[i].bytes + 255) / 256 * 256;
    }
    EXPECT(lay.total == sum);
    EXPECT(lay.total % 256 == 0);
}

int main() {
    check("no outputs", {});
    check("all null", {{false, 100}, {false, 0}, {false, 4096}});
    check("one byte", {{true, 1}});
    check("255", {{true, 255}, {true, 255}});
    check("256", {{true, 256}, {true, 256}});
    check("257", {{true, 257}, {true, 257}});
    check("255 256 257", {{true, 255}, {true, 256}, {true, 257}, {true, 1}});
    check("a null between two", {{true, 300}, {false, 300}, {true, 300}});
    check("an input, then outputs", {{true, 24 * 7}, {true, 4 * 7}, {false, 4 * 7}, {true, 12 * 7}, {false, 12 * 7}, {true, 12 * 7}});
    check("eight items", {{true, 12}, {true, 12}, {false, 8}, {true, 36}, {true, 24}, {false, 8}, {true, 4}, {true, 4}});
    // more than eight: the 21 arrays of a rollouts call with movers on a 37 x 19 grid (703 cells), 5 poses, 35 candidates each and
    // 9 steps, with cost, targets, three of the outputs and one of the movers' outputs NULL
    {
        const size_t P = 37 * 19, np = 5, NK = 5 * 35, traj = 5 * (9 + 1) * 3;
        check("a rollouts call", {{true, P}, {true, 4 * P}, {false, 4 * P}, {true, 12 * np}, {false, 8 * np},
                                  {true, 4 * np}, {true, 8 * np}, {false, 8 * np}, {true, 4 * np}, {true, 4 * np}, {true, 4 * np}, {true, 4 * traj},
                                  {true, 4 * NK}, {false, 4 * NK}, {true, 12 * NK}, {false, 4 * NK}, {true, 8 * NK},
                                  {true, 24 * 3}, {true, 4 * NK}, {false, 4 * NK}, {true, 4 * np}});
    }
    {
        std::vector<Decl> all((size_t)ssf::StageLayout::MAX_ITEMS);
        for (size_t i = 0; i < all.size(); i++) all[i] = Decl{i % 5 != 3, 100 * i + 1};
        check("every item, every fifth NULL", all);
    }
    {   // one item more than MAX_ITEMS is refused and changes nothing
        const char* what = "full";
        static const char host_byte = 0;
        ssf::StageLayout lay;
        for (int i = 0; i < ssf::StageLayout::MAX_ITEMS; i++) EXPECT(lay.add(&host_byte, 10) == i);
        const size_t total = lay.total;
        EXPECT(lay.add(&host_byte, 10) == -1);
        EXPECT(lay.n == ssf::StageLayout::MAX_ITEMS && lay.total == total);
    }
    if (failures) { std::printf("stage_layout_smoke: %d failures\n", failures); return 1; }
    std::printf("stage_layout_smoke ok\n");
    return 0;
}
