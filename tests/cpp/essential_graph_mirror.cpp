// Exercises cubeslam::build_essential_graph and, built with -DWITH_DEVICE, cubeslam::OptimizeEssentialGraph (cube_slam_amd/host/essential_graph.hpp) on a flattened map read
// from a text file (tests/test_essential_graph_mirrors.py::write_flat).  Prints the edge arrays, and with the device the bytes of sim3 / Tiw / points and the trial sequence.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "cube_slam_amd/host/essential_graph.hpp"

template <class T> static void hex(const std::vector<T> &v) {
    for (const T &x : v) { const unsigned char *b = reinterpret_cast<const unsigned char *>(&x); for (size_t k = 0; k < sizeof(T); k++) printf("%02x", b[k]); }
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 3;
    cubeslam::FlatMap m;
    size_t n, n_bad, n_lc, n_nc, np;
    int fix;
    f >> n >> m.loop_kf >> m.cur_kf >> fix >> n_bad >> n_lc;
    auto list = [&](std::vector<long> &v) { size_t c; f >> c; v.resize(c); for (long &x : v) f >> x; };
    m.kfs.resize(n);
    for (auto &kf : m.kfs) {
        int bad; size_t nw;
        f >> kf.mnId >> bad >> kf.parent;
        kf.bad = bad != 0;
        list(kf.loop_edges); list(kf.covisibles); list(kf.children);
        f >> nw;
        for (size_t k = 0; k < nw; k++) { long id; int w; f >> id >> w; kf.weights[id] = w; }
    }
    for (size_t k = 0; k < n_bad; k++) { long id; f >> id; m.bad.insert(id); }
    m.loop_connections.resize(n_lc);
    for (auto &lc : m.loop_connections) { f >> lc.first; list(lc.second); }
    for (size_t k = 0; k < n; k++) { long id; f >> id; std::vector<double> s(8); for (double &x : s) f >> x; m.Scw[id] = s; }
    f >> n_nc;
    for (size_t k = 0; k < n_nc; k++) { long id; f >> id; std::vector<double> s(8); for (double &x : s) f >> x; m.non_corrected[id] = s; }
    f >> np;
    std::vector<double> P(np * 3);
    std::vector<long> nIDr(np);
    for (size_t k = 0; k < np; k++) f >> P[k * 3] >> P[k * 3 + 1] >> P[k * 3 + 2] >> nIDr[k];
    if (!f) return 3;
    try {
#ifdef WITH_DEVICE
        cubeslam::Context ctx(0);
        const cubeslam::EssentialGraphResult res = cubeslam::OptimizeEssentialGraph(ctx, m, fix != 0, P, nIDr);
        const cubeslam::EssentialGraph &g = res.graph;
#else
        const cubeslam::EssentialGraph g = cubeslam::build_essential_graph(m);
#endif
        printf("fixed %d\n", g.fixed_vertex);
        hex(g.mnId); hex(g.edge_i); hex(g.edge_j); hex(g.edge_kind); hex(g.Scw); hex(g.Snc); hex(g.has_nc);
#ifdef WITH_DEVICE
        hex(res.sim3); hex(res.Tiw); hex(res.points);
        for (int k = 0; k < res.stats.trials; k++) printf("%d", (int)res.stats.trial_accepted[k]);
        printf("\n");
#endif
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
