// klt_handle.h -- the KLT handle as klt.hip (pyramids, tracker) and gftt.hip (corner detection on the resident level 0) share it
#pragma once
#include "common.h"
#include "klt_math.h"

// the temporaries of the corner detector; they grow to what a call needs and stay with their owner
struct GfttBufs {
    cs_dbuf<float> eig, corners, quality, pts;
    cs_dbuf<unsigned long long> keys;
    cs_dbuf<uint8_t> masks, good;
    cs_dbuf<int> ints;
};

struct cs_klt {
    int max_frames = 0, max_w = 0, max_h = 0, max_points = 0;
    cs_owner own;
    uint8_t *d_gray = nullptr, *d_img = nullptr, *d_status = nullptr;
    short *d_der = nullptr;
    float *d_prev = nullptr, *d_next = nullptr, *d_err = nullptr;
    int n_frames = 0, W = 0, H = 0;
    KltLayout L{};
    GfttBufs gftt;
};
