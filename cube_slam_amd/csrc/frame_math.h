// frame_math.h -- Frame::UndistortKeyPoints' point arithmetic, shared by match.hip (match_undistort, cs_frame_image_bounds) and rgbd.hip (the RGB-D gather).
#pragma once

// cv::undistortPoints(src, dst, K, D, Mat(), K) as Frame::UndistortKeyPoints / ComputeImageBounds call it (Frame.cc:546-609): the
// classic cvUndistortPoints of OpenCV 2.4 - 3.2 -- normalise with the double copies of the float intrinsics, five fixed-point
// iterations of the Brown model (k1 k2 p1 p2 k3), re-project with P = K, round to float.  (Later OpenCV versions stop the iteration on
// a reprojection-error criterion; the reference's target version is not pinned)  -ffp-contract=off: plain double ops.
struct UndP { double fx, fy, cx, cy, k[5]; int identity; };
__host__ __device__ inline void undistort_point(const UndP &U, float xin, float yin, float &xo, float &yo) {
    if (U.identity) { xo = xin; yo = yin; return; }
    const double ifx = 1. / U.fx, ify = 1. / U.fy;
    double x = ((double)xin - U.cx) * ifx, y = ((double)yin - U.cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2) / (1 + ((U.k[4] * r2 + U.k[1]) * r2 + U.k[0]) * r2);
        const double deltaX = 2 * U.k[2] * x * y + U.k[3] * (r2 + 2 * x * x);
        const double deltaY = U.k[2] * (r2 + 2 * y * y) + 2 * U.k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = U.fx * x + 0.0 * y + U.cx, yy = 0.0 * x + U.fy * y + U.cy, ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    xo = (float)(xx * ww); yo = (float)(yy * ww);
}

static UndP make_undp(const float *K4, const float *dist5) {
    UndP U; U.fx = K4[0]; U.fy = K4[1]; U.cx = K4[2]; U.cy = K4[3];
    for (int i = 0; i < 5; i++) U.k[i] = dist5 ? (double)dist5[i] : 0.0;
    U.identity = !dist5 || dist5[0] == 0.0f; // Frame.cc:548: only the first coefficient is looked at
    return U;
}
