// Driver of cube_slam_amd/host/bow.hpp for tests/test_bow_mirrors.py (mode "host": the text loader, the refusals and the candidate logic, no device) and
// tests/test_bow_host_cpp_gpu.py (mode "device": everything through the C-ABI).  Reads a script of one command per line and prints one answer per line:
//   voc <file> <levelsup>        -> voc <loaded> <k> <L> <scoring> <weighting> <n_nodes> <fnv of parent, is_leaf, desc, weight> <refused>      (device: also creates it)
//   frame <hex descriptors|->    -> bow <w:bits,...|-> fv <node:i.i.i,...|-> node <n,n,...|->                                                    (device)
//   score <bow> <bow>            -> score <bits>                                                                                                  (device)
//   add <id> <bow> | erase <id> | clear | newdb (a fresh database and fresh key-frame fields)                                                     (no answer)
//   loop <qid> <minScore float bits> <connected a,b|-> <cov k=a.b;k=c|-> <bow>   /   reloc <qid> <cov> <bow>      -> cand <a,b,...|->              (device)
//   cloop <qid> <minScore bits> <connected> <cov> <shared id.common.minword.order.scorebits,...|->   /   creloc <qid> <cov> <shared>   -> cand ...  (host)
// bow = w:bits,w:bits,... with the double as 16 hex digits.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "cube_slam_amd/host/bow.hpp"

using namespace cubeslam;

static std::vector<std::string> split(const std::string &s, char c) {
    std::vector<std::string> out;
    if (s == "-" || s.empty()) return out;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, c)) out.push_back(t);
    return out;
}
static double from_bits(const std::string &h) { uint64_t u = std::stoull(h, nullptr, 16); double d; memcpy(&d, &u, 8); return d; }
static float float_from_bits(const std::string &h) { uint32_t u = (uint32_t)std::stoul(h, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
static std::string bits(double d) { uint64_t u; memcpy(&u, &d, 8); char b[17]; snprintf(b, sizeof b, "%016" PRIx64, u); return b; }
static BowVector bow_of(const std::string &s) {
    BowVector b;
    for (const auto &e : split(s, ',')) { const auto p = split(e, ':'); b[std::stoi(p[0])] = from_bits(p[1]); }
    return b;
}
static Covisibles cov_of(const std::string &s) {
    Covisibles c;
    for (const auto &e : split(s, ';')) {
        const size_t q = e.find('=');
        auto &v = c[std::stol(e.substr(0, q))];
        for (const auto &x : split(e.substr(q + 1), '.')) v.push_back(std::stol(x));
    }
    return c;
}
static std::set<long> ids_of(const std::string &s) {
    std::set<long> o;
    for (const auto &x : split(s, ',')) o.insert(std::stol(x));
    return o;
}
static void print_cand(const std::vector<long> &c) {
    printf("cand ");
    if (c.empty()) printf("-");
    for (size_t i = 0; i < c.size(); ++i) printf("%s%ld", i ? "," : "", c[i]);
    printf("\n");
}
static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t *)p)[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const bool device = std::string(argv[1]) == "device";
    std::ifstream script(argv[2]);
    Context *ctx = device ? new Context(0) : nullptr;
    ORBVocabulary *voc = nullptr;
    KeyFrameDatabase *db = device ? new KeyFrameDatabase(*ctx) : nullptr;
    KeyFrameState state;
    std::string line;
    while (std::getline(script, line)) {
        std::stringstream ss(line);
        std::vector<std::string> t;
        for (std::string x; ss >> x;) t.push_back(x);
        if (t.empty()) continue;
        if (t[0] == "voc") {
            std::ifstream f(t[1].c_str());
            VocabularyArrays a;
            const bool loaded = f && parseVocabularyText(f, a);
            uint64_t h = 14695981039346656037ull;
            h = fnv(h, a.parent.data(), a.parent.size() * 4); h = fnv(h, a.is_leaf.data(), a.is_leaf.size()); h = fnv(h, a.desc.data(), a.desc.size());
            h = fnv(h, a.weight.data(), a.weight.size() * 8);
            const bool refused = !loaded || a.refused(std::stoi(t[2]));
            printf("voc %d %d %d %d %d %d %016" PRIx64 " %d\n", (int)loaded, a.k, a.L, a.scoring, a.weighting, a.n_nodes(), h, (int)refused);
            if (device && !refused) { delete voc; voc = new ORBVocabulary(*ctx, std::stoi(t[2])); voc->create(a); }
        } else if (t[0] == "frame") {
            std::vector<uint8_t> d;
            if (t[1] != "-")
                for (size_t i = 0; i + 1 < t[1].size(); i += 2) d.push_back((uint8_t)std::stoul(t[1].substr(i, 2), nullptr, 16));
            BowVector b;
            FeatureVector fv;
            std::vector<int> node;
            voc->transform(d, b, fv, std::stoi(t[2]), &node);
            printf("bow ");
            if (b.empty()) printf("-");
            for (auto it = b.begin(); it != b.end(); ++it) printf("%s%d:%s", it == b.begin() ? "" : ",", it->first, bits(it->second).c_str());
            printf(" fv ");
            if (fv.empty()) printf("-");
            for (auto it = fv.begin(); it != fv.end(); ++it) {
                printf("%s%d:", it == fv.begin() ? "" : ",", it->first);
                for (size_t i = 0; i < it->second.size(); ++i) printf("%s%u", i ? "." : "", it->second[i]);
            }
            printf(" node ");
            if (node.empty()) printf("-");
            for (size_t i = 0; i < node.size(); ++i) printf("%s%d", i ? "," : "", node[i]);
            printf("\n");
        } else if (t[0] == "score") {
            printf("score %s\n", bits(voc->score(bow_of(t[1]), bow_of(t[2]))).c_str());
        } else if (t[0] == "add") {
            db->add(std::stol(t[1]), bow_of(t[2]));
        } else if (t[0] == "newdb") {
            if (device) { delete db; db = new KeyFrameDatabase(*ctx); }
            state.clear();
        } else if (t[0] == "erase") {
            db->erase(std::stol(t[1]));
        } else if (t[0] == "clear") {
            db->clear();
        } else if (t[0] == "loop") {
            print_cand(db->DetectLoopCandidates(std::stol(t[1]), bow_of(t[5]), ids_of(t[3]), cov_of(t[4]), float_from_bits(t[2])));
        } else if (t[0] == "reloc") {
            print_cand(db->DetectRelocalizationCandidates(std::stol(t[1]), bow_of(t[3]), cov_of(t[2])));
        } else if (t[0] == "cloop" || t[0] == "creloc") {
            const bool loop = t[0] == "cloop";
            std::vector<SharedWords> sh;
            for (const auto &e : split(t[loop ? 5 : 3], ',')) {
                const auto p = split(e, '.');
                sh.push_back({std::stol(p[0]), std::stoi(p[1]), std::stoi(p[2]), std::stol(p[3]), from_bits(p[4])});
            }
            print_cand(loop ? DetectLoopCandidatesFromShared(state, sh, std::stol(t[1]), ids_of(t[3]), cov_of(t[4]), float_from_bits(t[2]))
                            : DetectRelocalizationCandidatesFromShared(state, sh, std::stol(t[1]), cov_of(t[2])));
        } else {
            fprintf(stderr, "unknown command %s\n", t[0].c_str());
            return 3;
        }
    }
    delete db; delete voc; delete ctx;
    return 0;
}
