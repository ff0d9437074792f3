// CPU emulation of the list-free formulation of DistributeOctTree that the device kernel orb_quadtree uses (a split pass =
// [children of the last expandable node n4..n1, ..., of the first] ++ [non-expandable nodes in order]; second phase with a push
// stack + deletion marks), checked against the sequential host restatement (cs_orb_host::QuadTree) on random inputs and on the
// families natural textures do not produce: lattices whose responses all tie, lattices with a cluster or with close pairs, points
// in one quadrant of one root, none / one / two points or a quota of 0 / 1 / 2, one to six root nodes.  par_distribute also mirrors
// the kernel's pool arithmetic (CAPN = 12N+64 node records, CAPL = 4N+16 list entries, CAPV = N+8 (size, id) entries) and reports
// the high-water mark of each quantity the kernel tests, as a fraction of its cap.
#include "cube_slam_amd/csrc/orb_quadtree.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using cs_orb_host::Cand;

struct PNode { int x0, y0, x1, y1, begin, end; bool no_more; };

// The quantities orb_quadtree compares with its caps, each at the place the kernel compares it: a value above its cap is where the kernel raises status = 1.
struct Pools {
    int nodes = 0; // n_nodes + T (first phase), nn + kk (second phase)                                   against CAPN
    int list = 0;  // T + n_keep (a first-phase list), nfront + kk (the second phase's pushed children)    against CAPL
    int vk = 0;    // nE + 1, nV + 1 (the kernel tests >= CAPV), nvn + kk (the second phase's next round)  against CAPV
    void see(int n_nodes, int n_list, int n_vk) { nodes = std::max(nodes, n_nodes); list = std::max(list, n_list); vk = std::max(vk, n_vk); }
};

static void par_distribute(const Cand *K, int n, int minX, int maxX, int minY, int maxY, int N, std::vector<int> &result, Pools *pools = nullptr) {
    result.clear();
    const int nIni = (int)std::round(static_cast<float>(maxX - minX) / (maxY - minY));
    if (nIni < 1 || n == 0) return;
    const float hX = static_cast<float>(maxX - minX) / nIni;
    std::vector<PNode> nodes;
    std::vector<int> perm(n), tmp(n);
    // roots: stable bucket by x / hX
    std::vector<int> cnt(nIni + 1, 0), bk(n);
    for (int i = 0; i < n; i++) { int b = (int)(K[i].x / hX); if (b >= nIni) b = nIni - 1; bk[i] = b; cnt[b + 1]++; }
    for (int b = 0; b < nIni; b++) cnt[b + 1] += cnt[b];
    { std::vector<int> pos(cnt.begin(), cnt.end() - 1); for (int i = 0; i < n; i++) perm[pos[bk[i]]++] = i; }
    std::vector<int> list; // node ids in list order
    for (int b = 0; b < nIni; b++) {
        PNode nd{(int)(hX * static_cast<float>(b)), 0, (int)(hX * static_cast<float>(b + 1)), maxY - minY, cnt[b], cnt[b + 1], false};
        if (nd.end == nd.begin) continue;
        nd.no_more = (nd.end - nd.begin) == 1;
        nodes.push_back(nd); list.push_back((int)nodes.size() - 1);
    }
    auto split = [&](int id, int cid[4], int csz[4]) { // creates children (ids in n1..n4 order, -1 if empty)
        const PNode nd = nodes[id];
        const int halfX = (int)std::ceil(static_cast<float>(nd.x1 - nd.x0) / 2), halfY = (int)std::ceil(static_cast<float>(nd.y1 - nd.y0) / 2);
        const int mx = nd.x0 + halfX, my = nd.y0 + halfY;
        int c[4] = {0, 0, 0, 0};
        std::vector<int> q(nd.end - nd.begin);
        for (int p = nd.begin; p < nd.end; p++) { const Cand &k = K[perm[p]]; q[p - nd.begin] = (k.x < mx) ? ((k.y < my) ? 0 : 2) : ((k.y < my) ? 1 : 3); c[q[p - nd.begin]]++; }
        int off[4] = {nd.begin, nd.begin + c[0], nd.begin + c[0] + c[1], nd.begin + c[0] + c[1] + c[2]}, pos[4] = {off[0], off[1], off[2], off[3]};
        for (int p = nd.begin; p < nd.end; p++) tmp[pos[q[p - nd.begin]]++] = perm[p];
        for (int p = nd.begin; p < nd.end; p++) perm[p] = tmp[p];
        const int bx[4][4] = {{nd.x0, nd.y0, mx, my}, {mx, nd.y0, nd.x1, my}, {nd.x0, my, mx, nd.y1}, {mx, my, nd.x1, nd.y1}};
        for (int k = 0; k < 4; k++) {
            cid[k] = -1; csz[k] = c[k];
            if (!c[k]) continue;
            nodes.push_back(PNode{bx[k][0], bx[k][1], bx[k][2], bx[k][3], off[k], off[k] + c[k], c[k] == 1});
            cid[k] = (int)nodes.size() - 1;
        }
    };
    std::vector<std::pair<int, int>> vsize; // (size, id) in creation order
    bool finish = false;
    while (!finish) {
        const int prev_size = (int)list.size();
        // ---- phase-1 pass, data-parallel form: new list = [children of the last expandable node reversed, ..., of the first reversed] ++ [non-expandable nodes in order]
        std::vector<int> expandable, keep;
        for (int id : list) (nodes[id].no_more ? keep : expandable).push_back(id);
        vsize.clear();
        int n_to_expand = 0;
        std::vector<std::vector<int>> kids(expandable.size());
        for (size_t e = 0; e < expandable.size(); e++) { // creation order = list order of the parents, n1..n4
            int cid[4], csz[4];
            split(expandable[e], cid, csz);
            for (int k = 0; k < 4; k++) if (cid[k] >= 0) { kids[e].push_back(cid[k]); if (csz[k] > 1) { n_to_expand++; vsize.push_back({csz[k], cid[k]}); } }
        }
        std::vector<int> nl;
        for (int e = (int)expandable.size() - 1; e >= 0; e--) for (int k = (int)kids[e].size() - 1; k >= 0; k--) nl.push_back(kids[e][k]);
        nl.insert(nl.end(), keep.begin(), keep.end());
        list.swap(nl);
        const int size = (int)list.size();
        if (pools) pools->see((int)nodes.size(), size, (int)expandable.size() + 1);
        if (size >= N || size == prev_size) finish = true;
        else if (size + n_to_expand * 3 > N) {
            if (pools) pools->see(0, 0, (int)vsize.size() + 1);
            // ---- phase 2: sequential, largest first.  list as: front (pushed children, newest first) ++ base with deletions
            std::vector<int> front; // push order; list order = reversed(front) ++ base(alive)
            std::vector<char> dead(nodes.size() * 8 + 64, 0);
            int cur = size;
            while (!finish) {
                const int ps = cur;
                auto prev = vsize;
                vsize.clear();
                int nvn = 0; // entries of the next round's (size, id) list, counted like the kernel: the test comes before the append
                std::sort(prev.begin(), prev.end());
                for (int j = (int)prev.size() - 1; j >= 0; j--) {
                    int cid[4], csz[4];
                    const int id = prev[j].second;
                    split(id, cid, csz);
                    if (dead.size() < nodes.size() + 8) dead.resize(nodes.size() * 2 + 64, 0);
                    { int kk = 0; for (int k = 0; k < 4; k++) kk += cid[k] >= 0; if (pools) pools->see((int)nodes.size(), (int)front.size() + kk, nvn + kk); }
                    for (int k = 0; k < 4; k++) if (cid[k] >= 0) { front.push_back(cid[k]); cur++; if (csz[k] > 1) { vsize.push_back({csz[k], cid[k]}); nvn++; } }
                    dead[id] = 1; cur--;
                    if (cur >= N) break;
                }
                if (cur >= N || cur == ps) finish = true;
            }
            std::vector<int> fl;
            for (int k = (int)front.size() - 1; k >= 0; k--) if (!dead[front[k]]) fl.push_back(front[k]);
            for (int id : list) if (!dead[id]) fl.push_back(id);
            list.swap(fl);
        }
    }
    for (int id : list) {
        const PNode &nd = nodes[id];
        int best = perm[nd.begin]; float mxr = K[best].response;
        for (int p = nd.begin + 1; p < nd.end; p++) if (K[perm[p]].response > mxr) { best = perm[p]; mxr = K[best].response; }
        result.push_back(best);
    }
}

// ---- input families.  Coordinates are integers in [0, W) x [0, H), distinct unless a family says otherwise, in raster order (the order the cell pass emits within a cell).
struct Family { const char *name; int trials = 0, bad = 0, over = 0; double fn = 0, fl = 0, fv = 0; };

static void lattice(std::vector<Cand> &K, int W, int H, int sx, int sy, int ox, int oy, float resp) {
    for (int y = oy; y < H; y += sy) for (int x = ox; x < W; x += sx) K.push_back(Cand{(float)x, (float)y, resp});
}
static void raster_sort(std::vector<Cand> &K) {
    std::stable_sort(K.begin(), K.end(), [](const Cand &a, const Cand &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
    K.erase(std::unique(K.begin(), K.end(), [](const Cand &a, const Cand &b) { return a.x == b.x && a.y == b.y; }), K.end());
}

static void run_case(Family &F, cs_orb_host::QuadTree &qt, const std::vector<Cand> &K, int W, int H, int N) {
    std::vector<int> a, b;
    Pools P;
    const int n = (int)K.size();
    qt.distribute(K.data(), n, 16, 16 + W, 16, 16 + H, N, a);
    par_distribute(K.data(), n, 16, 16 + W, 16, 16 + H, N, b, &P);
    F.trials++;
    if (a != b) { if (F.bad < 3) printf("MISMATCH %s: n=%d N=%d W=%d H=%d  sizes %zu %zu\n", F.name, n, N, W, H, a.size(), b.size()); F.bad++; }
    const int nIni = (int)std::round((float)W / H);
    if (nIni > 4) return; // the kernel hands these to the host before it touches a pool
    const int CAPN = 12 * std::max(N, 1) + 64, CAPL = 4 * N + 16, CAPV = N + 8;
    if (P.nodes > CAPN || P.list > CAPL || P.vk > CAPV) { if (F.over < 3) printf("OVER CAP %s: n=%d N=%d W=%d H=%d  nodes %d/%d list %d/%d vk %d/%d\n", F.name, n, N, W, H, P.nodes, CAPN, P.list, CAPL, P.vk, CAPV); F.over++; }
    F.fn = std::max(F.fn, (double)P.nodes / CAPN); F.fl = std::max(F.fl, (double)P.list / CAPL); F.fv = std::max(F.fv, (double)P.vk / CAPV);
}

int main() {
    cs_orb_host::QuadTree qt;
    std::vector<Family> fams;
    { // the original 3000 random trials (random coordinates, coincident points included, responses rng() % 50)
        std::mt19937 rng(7);
        Family F{"random"};
        for (int trial = 0; trial < 3000; trial++) {
            const int W = 100 + rng() % 1200, H = 60 + rng() % 500;
            const int n = rng() % 3 == 0 ? rng() % 40 : rng() % 6000;
            const int N = 1 + rng() % 600;
            std::vector<Cand> K(n);
            const bool clustered = rng() % 2;
            for (auto &k : K) {
                if (clustered && rng() % 3) { k.x = (float)(W / 3 + rng() % std::max(1, W / 10)); k.y = (float)(H / 2 + rng() % std::max(1, H / 10)); }
                else { k.x = (float)(rng() % W); k.y = (float)(rng() % H); }
                k.response = (float)(rng() % 50);
            }
            run_case(F, qt, K, W, H, N);
        }
        fams.push_back(F);
    }
    std::mt19937 rng(11);
    // every family below draws its frame with one to six root nodes (W = nIni * H + a little) and its quota from far below to above the point count
    auto frame = [&](int &W, int &H, int &nIni) { nIni = 1 + rng() % 6; H = 80 + rng() % 300; W = nIni * H + (int)(rng() % (H / 4)) - H / 8; };
    auto quota = [&](int n) { const int c[6] = {std::max(1, n / 16), std::max(1, n / 4), std::max(1, n / 2), std::max(1, n - 1), n + 1, 2 * n + 3}; return std::min(c[rng() % 6], 2600); };
    {
        Family F{"lattice, all responses equal"};
        for (int t = 0; t < 1500; t++) {
            int W, H, nIni; frame(W, H, nIni);
            std::vector<Cand> K;
            const int s = 2 + rng() % 14;
            lattice(K, W, H, s, rng() % 4 ? s : 2 + rng() % 14, rng() % s, rng() % s, 30.f);
            run_case(F, qt, K, W, H, quota((int)K.size()));
        }
        fams.push_back(F);
    }
    {
        Family F{"lattice with one cluster"};
        for (int t = 0; t < 1500; t++) {
            int W, H, nIni; frame(W, H, nIni);
            std::vector<Cand> K;
            const int s = 6 + rng() % 20, cw = 8 + rng() % 60, ch = 8 + rng() % 60, cx = rng() % std::max(1, W - cw), cy = rng() % std::max(1, H - ch);
            lattice(K, W, H, s, s, rng() % s, rng() % s, 30.f);
            for (int y = cy; y < cy + ch && y < H; y += 2) for (int x = cx; x < cx + cw && x < W; x += 2) K.push_back(Cand{(float)x, (float)y, 30.f});
            raster_sort(K);
            if (rng() % 2) for (auto &k : K) k.response = (float)(20 + rng() % 3); // few values: ties inside every node
            run_case(F, qt, K, W, H, quota((int)K.size()));
        }
        fams.push_back(F);
    }
    {
        Family F{"lattice of close pairs"}; // two points two pixels apart stay in one node for many splits: a split that creates one child adds a node and a list entry without adding to the count
        for (int t = 0; t < 1500; t++) {
            int W, H, nIni; frame(W, H, nIni);
            std::vector<Cand> K;
            const int s = 8 + rng() % 40, ox = rng() % s, oy = rng() % s, d = 2 + rng() % 2;
            for (int y = oy; y < H; y += s) for (int x = ox; x + d < W; x += s) { K.push_back(Cand{(float)x, (float)y, 30.f}); K.push_back(Cand{(float)(x + d), (float)y, 30.f}); }
            run_case(F, qt, K, W, H, quota((int)K.size()));
        }
        fams.push_back(F);
    }
    {
        Family F{"one quadrant of one root"};
        for (int t = 0; t < 1500; t++) {
            int W, H, nIni; frame(W, H, nIni);
            const int rw = W / nIni, root = rng() % nIni, qx = rng() % 2, qy = rng() % 2;
            const int x0 = root * rw + qx * (rw / 2) + 1, y0 = qy * (H / 2) + 1, bw = rw / 2 - 2, bh = H / 2 - 2;
            std::vector<Cand> K;
            if (rng() % 2) { const int s = 2 + rng() % 6; for (int y = y0; y < y0 + bh; y += s) for (int x = x0; x < x0 + bw; x += s) K.push_back(Cand{(float)x, (float)y, 30.f}); }
            else { const int n = 1 + rng() % 800; for (int i = 0; i < n; i++) K.push_back(Cand{(float)(x0 + rng() % bw), (float)(y0 + rng() % bh), (float)(20 + rng() % 2)}); raster_sort(K); }
            run_case(F, qt, K, W, H, quota((int)K.size()));
        }
        fams.push_back(F);
    }
    {
        Family F{"0, 1 or 2 points; quota 0, 1 or 2"};
        for (int t = 0; t < 1500; t++) {
            int W, H, nIni; frame(W, H, nIni);
            std::vector<Cand> K;
            const bool few_points = t % 2;
            const int n = few_points ? t / 2 % 3 : 1 + rng() % 500;
            for (int i = 0; i < n; i++) K.push_back(Cand{(float)(rng() % W), (float)(rng() % H), (float)(20 + rng() % 2)});
            raster_sort(K);
            run_case(F, qt, K, W, H, few_points ? 1 + rng() % 50 : t / 2 % 3);
        }
        fams.push_back(F);
    }
    int bad = 0, over = 0;
    double top = 0;
    for (const Family &F : fams) {
        printf("%-36s %5d trials  %d mismatches  %d over a cap  high water: nodes %.3f of CAPN, lists %.3f of CAPL, (size, id) %.3f of CAPV\n", F.name, F.trials, F.bad, F.over, F.fn, F.fl, F.fv);
        bad += F.bad; over += F.over; top = std::max(top, std::max(F.fn, std::max(F.fl, F.fv)));
    }
    printf("highest fraction of a cap: %.3f (%d cases over a cap)\n", top, over);
    printf("%s (%d mismatches)\n", bad ? "FAIL" : "all equal", bad);
    return bad != 0;
}
