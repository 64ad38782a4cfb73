// klt.h — the device-resident image of klt.hip (rs_image), shared with the other stages that read its pyramid
// (gftt.hip reads level 0).  Layout: klt.hip's header comment.
#pragma once
#include "common.h"

#define KLT_MAX_LEVELS 7
#define KLT_MAX_DIM 4096
#define KLT_MAX_POINTS 8192

struct KltLevel {
    int w, h, pitch, rows;          // interior size, padded pitch (elements), padded rows
    uint8_t* img;                   // padded base (pixel (-pad, -pad))
    short2* der;                    // padded base
};

struct KltPyr {
    int levels, pad;
    KltLevel lv[KLT_MAX_LEVELS];
};

struct rs_image {
    rs_context* ctx = nullptr;
    int width = 0, height = 0, max_level = 0, win = 0;
    KltPyr pyr{};
    rs_dev_block block;             // every level and d_stage
    uint8_t* d_stage = nullptr;     // raw upload of a host frame (width * height * 3 bytes)
    bool valid = false;             // a frame has been uploaded
};
