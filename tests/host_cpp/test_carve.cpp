// racing-slam_amd/csrc/carve.h on its own: one layout run on a null carver and on a malloc'ed block, as a stand-alone
// program under the address and undefined-behaviour sanitizers (tests/test_carve_cpu.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../racing-slam_amd/csrc/carve.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
    } while (0)

struct Wide { double a; int32_t b[3]; };   // 24 bytes: a count of it is no multiple of 256

struct Object {
    uint8_t* bytes1;        // [1]
    uint8_t* bytes256;      // [256]
    uint8_t* bytes257;      // [257]
    int32_t* ints;          // [65]
    double* doubles;        // [257]
    Wide* wide;             // [11]
    uint16_t* tail;         // [3]
};
struct Piece { char* p; size_t bytes; };

// the layout, stated once; `pieces` records what each take gave
static void layout(rs_carve& c, Object* o, std::vector<Piece>* pieces)
{
    pieces->clear();
    o->bytes1 = c.take<uint8_t>(1);         pieces->push_back({(char*)o->bytes1, 1});
    o->bytes256 = c.take<uint8_t>(256);     pieces->push_back({(char*)o->bytes256, 256});
    o->bytes257 = c.take<uint8_t>(257);     pieces->push_back({(char*)o->bytes257, 257});
    o->ints = c.take<int32_t>(65);          pieces->push_back({(char*)o->ints, sizeof(int32_t) * 65});
    o->doubles = c.take<double>(257);       pieces->push_back({(char*)o->doubles, sizeof(double) * 257});
    o->wide = c.take<Wide>(11);             pieces->push_back({(char*)o->wide, sizeof(Wide) * 11});
    o->tail = c.take<uint16_t>(3);          pieces->push_back({(char*)o->tail, sizeof(uint16_t) * 3});
}

int main()
{
    CHECK(rs_align256(0) == 0 && rs_align256(1) == 256 && rs_align256(255) == 256 && rs_align256(256) == 256 && rs_align256(257) == 512);

    // 1, 256 and 257 bytes advance by 256, 256 and 512
    {
        rs_carve c;
        CHECK(c.bytes() == 0);
        CHECK(c.take<uint8_t>(1) == nullptr && c.bytes() == 256);
        CHECK(c.take<uint8_t>(256) == nullptr && c.bytes() == 512);
        CHECK(c.take<uint8_t>(257) == nullptr && c.bytes() == 1024);
    }

    Object o;
    std::vector<Piece> pieces;
    rs_carve size;
    layout(size, &o, &pieces);
    for (const Piece& q : pieces) CHECK(q.p == nullptr);
    const size_t total = size.bytes();
    CHECK(total == 256 + 256 + 512 + 512 + 2304 + 512 + 256);

    // malloc gives 16-byte alignment: place on the first 256-byte boundary inside a block with that much room in front
    char* raw = (char*)malloc(total + 255);
    CHECK(raw != nullptr);
    if (!raw) return 1;
    char* base = raw + (rs_align256((size_t)(uintptr_t)raw) - (size_t)(uintptr_t)raw);
    rs_carve place(base);
    layout(place, &o, &pieces);
    CHECK(place.bytes() == total);                                       // the two runs agree

    const char* at = base;
    for (size_t i = 0; i < pieces.size(); i++) {
        CHECK(pieces[i].p != nullptr);
        CHECK(((uintptr_t)pieces[i].p & 255) == 0);                      // aligned
        CHECK(pieces[i].p >= at);                                        // in order, disjoint from the one before
        at = pieces[i].p + pieces[i].bytes;
    }
    CHECK(at <= base + total);                                           // the last piece ends inside the block
    CHECK(o.bytes256 - o.bytes1 == 256 && o.bytes257 - o.bytes256 == 256 && (char*)o.ints - (char*)o.bytes257 == 512);

    // every byte of every piece written with its piece index, then read back
    for (size_t i = 0; i < pieces.size(); i++) memset(pieces[i].p, (int)(i + 1), pieces[i].bytes);
    for (size_t i = 0; i < pieces.size(); i++)
        for (size_t k = 0; k < pieces[i].bytes; k++) CHECK((unsigned char)pieces[i].p[k] == i + 1);
    // and through the typed pointers
    o.ints[64] = -7; o.doubles[256] = 0.5; o.wide[10].b[2] = 9; o.tail[2] = 65535;
    CHECK(o.ints[64] == -7 && o.doubles[256] == 0.5 && o.wide[10].b[2] == 9 && o.tail[2] == 65535);
    free(raw);

    if (g_fail) { printf("%d carve checks FAILED\n", g_fail); return 1; }
    printf("carve checks passed\n");
    return 0;
}
