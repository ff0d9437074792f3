// TEST INFRASTRUCTURE: drives cubeslam::Tracking (cube_slam_amd/host/tracking.hpp) from a file of arrays and writes what it computed to another, for
// tests/test_track_local_map_mirrors.py (`host`: UpdateLocalKeyFrames alone, compiled with -DCUBESLAM_HOST_ONLY and nothing of the library) and
// tests/test_track_local_map_host_cpp_gpu.py (the whole TrackLocalMap over the C-ABI library).  An array in a file is an int64 byte count and the bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cube_slam_amd/host/tracking.hpp"

namespace {
struct Reader {
    FILE *f;
    template <class T> std::vector<T> next() {
        int64_t nb = 0;
        if (fread(&nb, 8, 1, f) != 1 || nb < 0 || nb % (int64_t)sizeof(T)) { fprintf(stderr, "bad input\n"); exit(2); }
        std::vector<T> v((size_t)nb / sizeof(T));
        if (nb && fread(v.data(), 1, (size_t)nb, f) != (size_t)nb) { fprintf(stderr, "short input\n"); exit(2); }
        return v;
    }
};
struct Writer {
    FILE *f;
    template <class T> void put(const std::vector<T> &v) { const int64_t nb = (int64_t)(v.size() * sizeof(T)); fwrite(&nb, 8, 1, f); if (nb) fwrite(v.data(), 1, (size_t)nb, f); }
};
void read_graph(Reader &in, std::vector<int> &frame_mp, cubeslam::TrackMap &m) {
    frame_mp = in.next<int>(); m.bad = in.next<uint8_t>(); m.obs_off = in.next<int>(); m.obs_kf = in.next<int>(); m.kf_bad = in.next<uint8_t>();
    m.cov_off = in.next<int>(); m.cov_kf = in.next<int>(); m.child_off = in.next<int>(); m.child_kf = in.next<int>(); m.parent = in.next<int>();
    m.dynamic.assign(m.bad.size(), 0);
}
} // namespace

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: tracking_mirror in.bin out.bin [host]\n"); return 2; }
    Reader in{fopen(argv[1], "rb")};
    Writer out{fopen(argv[2], "wb")};
    if (!in.f || !out.f) return 2;
    const bool host = argc > 3 && std::string(argv[3]) == "host";
    if (host) { // graphs until the input ends: UpdateLocalKeyFrames from a sentinel list
        const int n_graphs = in.next<int>()[0];
        for (int g = 0; g < n_graphs; g++) {
            std::vector<int> frame_mp; cubeslam::TrackMap m;
            read_graph(in, frame_mp, m);
#ifdef CUBESLAM_HOST_ONLY
            cubeslam::Tracking t;
            t.mvpLocalKeyFrames = {-7};
            t.UpdateLocalKeyFrames(frame_mp, m);
            out.put(t.mvpLocalKeyFrames);
            out.put(std::vector<int>{t.mpReferenceKF});
            out.put(frame_mp);
#endif
        }
        fclose(out.f);
        return 0;
    }
#ifndef CUBESLAM_HOST_ONLY
    cubeslam::TrackMap m; cubeslam::TrackFrame F;
    read_graph(in, F.mvpMapPoints, m);
    m.world_pos = in.next<float>(); m.normal = in.next<float>(); m.min_distance = in.next<float>(); m.max_distance = in.next<float>(); m.desc = in.next<uint8_t>(); m.n_obs = in.next<int>();
    m.kf_off = in.next<int>(); m.kf_mp = in.next<int>();
    m.last_frame_seen.assign(m.bad.size(), -1); m.visible.assign(m.bad.size(), 0); m.found.assign(m.bad.size(), 0);
    F.mvKeysUn = in.next<cs_keypoint>(); F.mDescriptors = in.next<uint8_t>();
    const std::vector<float> b = in.next<float>(), R = in.next<float>(), t = in.next<float>(), O = in.next<float>(), intr = in.next<float>();
    F.mnMinX = b[0]; F.mnMaxX = b[1]; F.mnMinY = b[2]; F.mnMaxY = b[3];
    memcpy(F.mRcw, R.data(), 36); memcpy(F.mtcw, t.data(), 12); memcpy(F.mOw, O.data(), 12);
    F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; F.mbf = intr[4]; F.mfLogScaleFactor = intr[5];
    F.mvScaleFactors = in.next<float>(); F.mvInvLevelSigma2 = in.next<float>();
    const std::vector<double> pose = in.next<double>();
    memcpy(F.pose, pose.data(), 56);
    F.mnId = in.next<int>()[0];
    cubeslam::Context c(0);
    cubeslam::Tracking T(c);
    const bool ok = T.TrackLocalMap(F, m);
    out.put(T.mvpLocalKeyFrames); out.put(T.mvpLocalMapPoints); out.put(T.train_match); out.put(T.in_view); out.put(T.pred_level); out.put(T.proj); out.put(T.view_cos);
    out.put(F.mvpMapPoints); out.put(F.mvbOutlier); out.put(std::vector<double>(F.pose, F.pose + 7));
    out.put(std::vector<int>{T.nmatches, T.nToMatch, T.n_level_outside, T.mnMatchesInliers, (int)ok, T.mpReferenceKF});
    out.put(m.visible); out.put(m.found);
#endif
    fclose(out.f);
    return 0;
}
