// bow.hip -- place recognition: the DBoW2 vocabulary transform (TemplatedVocabulary::transform, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1271),
// L1Scoring::score (ScoringObject.cpp:23-68) and the key-frame database behind KeyFrameDatabase::Detect*Candidates (src/KeyFrameDatabase.cc:74-305).
// Parity is bit-exact: the descent is integer Hamming arithmetic with the reference's tie rule (the first child wins), and every double is produced by the
// reference's own sequence of operations (no atomics, no tree reduction on doubles; -ffp-contract=off is the build's setting).
//
// Device layout of a vocabulary: the children of a node lie one behind the other ("slots", breadth first, file order inside a node), their
// descriptors first: slot_desc[slot] = 32 B, slot_node[slot] = node id.  Per node: node_first (its first child slot), node_nchild, node_word, node_weight.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int BOW_MAX_FRAME = 8192; // features of one frame the accumulation kernel sorts in LDS (32 KiB of keys)

// ---- descent: one lane group per feature, one lane per child ---------------------------------------------------------------------------------------------------------
// The six levels of a feature are a chain of dependent gathers of one child block each (k x 32 B, one coalesced load of the group); a wave holds 64 / GW chains and the
// occupancy hides the rest of the latency.  min over dist * 32 + child gives FORB::distance's strict `d < best_d` (the first child wins a tie) without a branch.
template <int GW>
__global__ __launch_bounds__(256) void bow_descend(const uint4 *__restrict__ slot_desc, const int *__restrict__ slot_node, const int *__restrict__ node_first,
                                                   const int *__restrict__ node_nchild, const int *__restrict__ node_word, const double *__restrict__ node_weight, int nid_level,
                                                   long n_feat, const uint4 *__restrict__ desc, int *__restrict__ word, int *__restrict__ node) {
    const long g = (blockIdx.x * 256L + threadIdx.x) / GW;
    const int c = threadIdx.x % GW;
    const bool live = g < n_feat;
    const long gi = live ? g : n_feat - 1; // a group past the end walks the last feature and stores nothing: every lane of a group takes the same path
    const uint4 f0 = desc[2 * gi], f1 = desc[2 * gi + 1];
    int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
    int nc = node_nchild[0];
    while (nc > 0) {
        ++level;
        const int first = node_first[cur];
        int key = INT_MAX;
        if (c < nc) {
            const uint4 a = slot_desc[2 * (long)(first + c)], b = slot_desc[2 * (long)(first + c) + 1];
            const int d = __popc(a.x ^ f0.x) + __popc(a.y ^ f0.y) + __popc(a.z ^ f0.z) + __popc(a.w ^ f0.w) + __popc(b.x ^ f1.x) + __popc(b.y ^ f1.y) + __popc(b.z ^ f1.z) +
                          __popc(b.w ^ f1.w);
            key = d * 32 + c;
        }
#pragma unroll
        for (int m = GW / 2; m > 0; m >>= 1) key = min(key, __shfl_xor(key, m, GW));
        cur = slot_node[first + (key & 31)];
        if (level == nid_level) nid = cur;
        nc = node_nchild[cur];
    }
    if (live && c == 0) {
        const bool kept = node_weight[cur] > 0; // "not stopped" (:1169)
        word[g] = kept ? node_word[cur] : -1;
        node[g] = kept ? nid : -1;
    }
}

// ---- accumulation: one workgroup per frame ---------------------------------------------------------------------------------------------------------------------------
// BowVector::addWeight adds the same w once per further occurrence of a word, so a word's value is the chain w + w + ... over its count; the counts come from a
// bitonic sort of the frame's words in LDS.  The L1 norm is one ordered chain over the words in ascending id (BowVector::normalize), then one division per word.
__global__ __launch_bounds__(256) void bow_accumulate(const int *__restrict__ offsets, const int *__restrict__ word, const double *__restrict__ word_weight, int P,
                                                      int *__restrict__ bow_count, int *__restrict__ bow_word, double *bow_value) {
    extern __shared__ int s[]; // P keys, then 256 scan cells
    int *scan = s + P;
    constexpr int NORM_BLOCK = 1024;
    __shared__ double norm_s, vbuf[NORM_BLOCK];
    const int f = blockIdx.x, t = threadIdx.x;
    const int o = offsets[f], n = offsets[f + 1] - o;
    for (int i = t; i < P; i += 256) {
        const int w = i < n ? word[o + i] : -1;
        s[i] = w < 0 ? INT_MAX : w;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const int a = s[i], b = s[x];
                    if ((a > b) == ((i & k2) == 0)) { s[i] = b; s[x] = a; }
                }
            }
            __syncthreads();
        }
    const int C = P / 256, lo_i = t * C, hi_i = lo_i + C;
    int cnt = 0;
    for (int i = lo_i; i < hi_i; ++i) cnt += s[i] != INT_MAX && (i == 0 || s[i] != s[i - 1]);
    scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) { // inclusive scan of the 256 counts
        const int add = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    int j = scan[t] - cnt;
    const int nu = scan[255];
    for (int i = lo_i; i < hi_i; ++i) {
        const int w = s[i];
        if (w == INT_MAX || (i > 0 && w == s[i - 1])) continue;
        int lo = i + 1, hi = P; // end of the run of w
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] == w) lo = mid + 1; else hi = mid;
        }
        const double wt = word_weight[w];
        double v = wt;
        for (int c = lo - i; c > 1; --c) v += wt;
        bow_word[o + j] = w;
        bow_value[o + j] = v;
        ++j;
    }
    __syncthreads();
    double nm0 = 0.0; // thread 0's chain; the values pass through LDS a block at a time so that the chain waits for no global load
    for (int base = 0; base < nu; base += NORM_BLOCK) {
        const int m = min(NORM_BLOCK, nu - base);
        for (int q = t; q < m; q += 256) vbuf[q] = fabs(bow_value[o + base + q]);
        __syncthreads();
        if (t == 0) {
            int q = 0;
            for (; q + 8 <= m; q += 8) { // eight LDS reads in flight in front of the eight dependent additions
                const double a0 = vbuf[q], a1 = vbuf[q + 1], a2 = vbuf[q + 2], a3 = vbuf[q + 3], a4 = vbuf[q + 4], a5 = vbuf[q + 5], a6 = vbuf[q + 6], a7 = vbuf[q + 7];
                nm0 += a0; nm0 += a1; nm0 += a2; nm0 += a3; nm0 += a4; nm0 += a5; nm0 += a6; nm0 += a7;
            }
            for (; q < m; ++q) nm0 += vbuf[q];
        }
        __syncthreads();
    }
    if (t == 0) { norm_s = nm0; bow_count[f] = nu; }
    __syncthreads();
    const double nm = norm_s;
    if (nm > 0.0)
        for (int q = t; q < nu; q += 256) bow_value[o + q] /= nm;
}

// ---- L1Scoring::score: one wave per pair -----------------------------------------------------------------------------------------------------------------------------
// Both lists are sorted: every lane looks one word of v1 up in v2, and the terms of the hits are added in lane order, which is ascending word id.
__device__ __forceinline__ double bow_score_wave(const int *__restrict__ aw, const double *__restrict__ av, int na, const int *__restrict__ bw, const double *__restrict__ bv, int nb,
                                                 int &common, int &minword) {
    const int lane = lane_id();
    double score = 0;
    common = 0;
    minword = -1;
    for (int base = 0; base < na; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double term = 0;
        int w = 0;
        if (i < na) {
            w = aw[i];
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bw[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nb && bw[lo] == w) {
                hit = true;
                const double vi = av[i], wi = bv[lo];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long m = __ballot(hit);
        if (m && minword < 0) minword = __shfl(w, __ffsll((long long)m) - 1);
        common += __popcll(m);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            score += __shfl(term, l);
        }
    }
    return -score / 2.0;
}

__global__ __launch_bounds__(256) void bow_query(int n_query, const int *__restrict__ q_off, const int *__restrict__ q_word, const double *__restrict__ q_value, int n_kf,
                                                 const long *__restrict__ kf_off, const int *__restrict__ kf_cnt, const int *__restrict__ pool_word,
                                                 const double *__restrict__ pool_value, int *__restrict__ common, int *__restrict__ minword, double *__restrict__ score) {
    const long p = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (p >= (long)n_query * n_kf) return;
    const int q = (int)(p / n_kf), k = (int)(p % n_kf);
    int c, mw;
    const double sc = bow_score_wave(q_word + q_off[q], q_value + q_off[q], q_off[q + 1] - q_off[q], pool_word + kf_off[k], pool_value + kf_off[k], kf_cnt[k], c, mw);
    if (lane_id() == 0) { common[p] = c; minword[p] = mw; score[p] = sc; }
}

__global__ __launch_bounds__(256) void bow_score_pairs(const int *__restrict__ off, const int *__restrict__ word, const double *__restrict__ value, int n_pairs,
                                                       const int *__restrict__ pa, const int *__restrict__ pb, double *__restrict__ score) {
    const long p = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const int a = pa[p], b = pb[p];
    int c, mw;
    const double sc = bow_score_wave(word + off[a], value + off[a], off[a + 1] - off[a], word + off[b], value + off[b], off[b + 1] - off[b], c, mw);
    if (lane_id() == 0) score[p] = sc;
}

bool csr_ok(int n, const int *off, const int *word) { // offsets from 0, not decreasing; words of a vector strictly ascending and >= 0
    if (off[0] != 0) return false;
    for (int i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return false;
        for (int j = off[i]; j < off[i + 1]; ++j)
            if (word[j] < 0 || (j > off[i] && word[j] <= word[j - 1])) return false;
    }
    return true;
}

} // namespace

struct cs_bow_vocab {
    cs_ctx *ctx = nullptr;
    cs_owner own;
    int k = 0, L = 0, n_nodes = 0, n_words = 0, levelsup = 0, max_children = 0;
    uint4 *d_slot_desc = nullptr;
    int *d_slot_node = nullptr, *d_node_first = nullptr, *d_node_nchild = nullptr, *d_node_word = nullptr;
    double *d_node_weight = nullptr, *d_word_weight = nullptr;
};

struct cs_bow_db {
    struct entry { long id; long seq; long off; int cnt; };
    cs_ctx *ctx = nullptr;
    cs_owner own;
    std::vector<entry> live; // in add order
    long next_seq = 0, used = 0, cap = 0, dead = 0;
    int *d_word = nullptr;
    double *d_value = nullptr;
};

extern "C" {

void cs_bow_vocab_destroy(cs_bow_vocab *v) {
    if (!v) return;
    v->own.free_all(v->ctx);
    delete v;
}

static const char *bow_vocab_refusal(int k, int L, int n_nodes, const int *parent, const uint8_t *is_leaf, int levelsup, int weighting, int scoring, std::vector<int> &nchild) {
    if (!parent || !is_leaf || n_nodes < 1) return "null array or no node";
    if (weighting != CS_BOW_TF_IDF || scoring != CS_BOW_L1_NORM) return "only TF_IDF weighting with L1 scoring is supported";
    if (k < 2 || k > 20 || L < 1 || L > 10) return "k outside 2..20 or L outside 1..10";
    std::vector<int> depth(n_nodes, 0);
    nchild.assign(n_nodes, 0);
    for (int i = 1; i < n_nodes; ++i) {
        if (parent[i] < 0 || parent[i] >= i) return "a parent id is not smaller than the node's own id";
        nchild[parent[i]]++;
        depth[i] = depth[parent[i]] + 1;
    }
    const int nid_level = L - levelsup;
    for (int i = 0; i < n_nodes; ++i) {
        if ((is_leaf[i] != 0) != (nchild[i] == 0)) return "a node's leaf flag disagrees with its having no children";
        if (nchild[i] == 0 && nid_level > 0 && depth[i] < nid_level) return "a leaf above level L - levelsup leaves the feature's node undefined";
        if (nchild[i] > k) return "a node with more than k children";
    }
    return nullptr;
}

int cs_bow_vocab_check(int k, int L, int n_nodes, const int *parent, const uint8_t *is_leaf, int levelsup, int weighting, int scoring) {
    std::vector<int> nchild;
    return bow_vocab_refusal(k, L, n_nodes, parent, is_leaf, levelsup, weighting, scoring, nchild) ? CS_ERR_BAD_ARG : CS_OK;
}

int cs_bow_vocab_create(cs_ctx *ctx, int k, int L, int n_nodes, const int *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight, int levelsup, int weighting,
                        int scoring, cs_bow_vocab **out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return CS_ERR_BAD_ARG;
    std::vector<int> nchild;
    const char *why = !desc || !weight ? "null array" : bow_vocab_refusal(k, L, n_nodes, parent, is_leaf, levelsup, weighting, scoring, nchild);
    if (why) { ctx->err = std::string("cs_bow_vocab_create: ") + why; return CS_ERR_BAD_ARG; }
    int max_children = 0, n_words = 0;
    for (int i = 0; i < n_nodes; ++i) max_children = std::max(max_children, nchild[i]);
    // slots: breadth first over the nodes in id order (a parent precedes its children), file order inside a node
    std::vector<int> first(n_nodes, 0), fill(n_nodes, 0), word(n_nodes, -1), slot_node(std::max(n_nodes - 1, 1), 0);
    int next = 0;
    for (int i = 0; i < n_nodes; ++i) { first[i] = next; next += nchild[i]; }
    std::vector<uint8_t> slot_desc((size_t)std::max(n_nodes - 1, 1) * 32, 0);
    std::vector<double> word_weight;
    for (int i = 0; i < n_nodes; ++i) {
        if (i > 0) {
            const int s = first[parent[i]] + fill[parent[i]]++;
            slot_node[s] = i;
            memcpy(&slot_desc[(size_t)s * 32], desc + (size_t)i * 32, 32);
        }
        if (is_leaf[i]) { word[i] = n_words++; word_weight.push_back(weight[i]); } // word ids in node-id order (:1421-1428)
    }
    cs_bow_vocab *v = new cs_bow_vocab;
    v->ctx = ctx; v->k = k; v->L = L; v->n_nodes = n_nodes; v->n_words = n_words; v->levelsup = levelsup; v->max_children = max_children;
    const size_t ns = slot_node.size();
    int r = v->own.alloc(ctx, &v->d_slot_desc, ns * 2);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_slot_node, ns);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_node_first, (size_t)n_nodes);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_node_nchild, (size_t)n_nodes);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_node_word, (size_t)n_nodes);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_node_weight, (size_t)n_nodes);
    if (r == CS_OK) r = v->own.alloc(ctx, &v->d_word_weight, word_weight.size());
    if (r == CS_OK) r = cs_h2d(ctx, (uint8_t *)v->d_slot_desc, slot_desc.data(), slot_desc.size());
    if (r == CS_OK) r = cs_h2d(ctx, v->d_slot_node, slot_node.data(), ns);
    if (r == CS_OK) r = cs_h2d(ctx, v->d_node_first, first.data(), (size_t)n_nodes);
    if (r == CS_OK) r = cs_h2d(ctx, v->d_node_nchild, nchild.data(), (size_t)n_nodes);
    if (r == CS_OK) r = cs_h2d(ctx, v->d_node_word, word.data(), (size_t)n_nodes);
    if (r == CS_OK) r = cs_h2d(ctx, v->d_node_weight, weight, (size_t)n_nodes);
    if (r == CS_OK) r = cs_h2d(ctx, v->d_word_weight, word_weight.data(), word_weight.size());
    if (r == CS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "cs_bow_vocab_create: upload failed"; r = CS_ERR_HIP; } // the host vectors above go out of scope
    if (r != CS_OK) { cs_bow_vocab_destroy(v); return r; }
    *out = v;
    return CS_OK;
}

int cs_bow_vocab_info(const cs_bow_vocab *v, int *k, int *L, int *n_nodes, int *n_words, int *levelsup) {
    if (!v) return CS_ERR_BAD_ARG;
    if (k) *k = v->k;
    if (L) *L = v->L;
    if (n_nodes) *n_nodes = v->n_nodes;
    if (n_words) *n_words = v->n_words;
    if (levelsup) *levelsup = v->levelsup;
    return CS_OK;
}

// the device part of cs_bow_transform; its blocks are released on every way out, after the stream has drained
static int bow_transform_dev(cs_ctx *ctx, const cs_bow_vocab *v, int n_frames, const int *offsets, const uint8_t *desc, int max_n, long n, int *word, int *node, int *bow_count,
                             int *bow_word, double *bow_value) {
    cs_scratch sc(ctx);
    uint4 *d_desc = nullptr;
    int *d_off = nullptr, *d_word = nullptr, *d_node = nullptr, *d_cnt = nullptr, *d_bw = nullptr;
    double *d_bv = nullptr;
    CS_TRY(sc.alloc(ctx, &d_desc, (size_t)n * 2)); CS_TRY(sc.alloc(ctx, &d_off, (size_t)n_frames + 1)); CS_TRY(sc.alloc(ctx, &d_word, (size_t)n)); CS_TRY(sc.alloc(ctx, &d_node, (size_t)n));
    CS_TRY(sc.alloc(ctx, &d_cnt, (size_t)n_frames)); CS_TRY(sc.alloc(ctx, &d_bw, (size_t)n)); CS_TRY(sc.alloc(ctx, &d_bv, (size_t)n));
    CS_TRY(cs_h2d(ctx, (uint8_t *)d_desc, desc, (size_t)n * 32)); CS_TRY(cs_h2d(ctx, d_off, offsets, (size_t)n_frames + 1));
    if (n > 0) {
        CS_HIP(ctx, hipMemsetAsync(d_bw, 0xff, (size_t)n * sizeof(int), ctx->stream)); // entries behind bow_count[f]: word -1, value 0
        CS_HIP(ctx, hipMemsetAsync(d_bv, 0, (size_t)n * sizeof(double), ctx->stream));
        const int nid_level = v->L - v->levelsup;
        if (v->max_children <= 16) {
            const unsigned grid = (unsigned)((n * 16 + 255) / 256);
            CS_LAUNCH(ctx, "bow_descend", bow_descend<16>, dim3(grid), dim3(256), 0, v->d_slot_desc, v->d_slot_node, v->d_node_first, v->d_node_nchild, v->d_node_word,
                      v->d_node_weight, nid_level, n, d_desc, d_word, d_node);
        } else {
            const unsigned grid = (unsigned)((n * 32 + 255) / 256);
            CS_LAUNCH(ctx, "bow_descend", bow_descend<32>, dim3(grid), dim3(256), 0, v->d_slot_desc, v->d_slot_node, v->d_node_first, v->d_node_nchild, v->d_node_word,
                      v->d_node_weight, nid_level, n, d_desc, d_word, d_node);
        }
    }
    int P = 256;
    while (P < max_n) P <<= 1;
    CS_LAUNCH(ctx, "bow_accumulate", bow_accumulate, dim3(n_frames), dim3(256), (size_t)(P + 256) * sizeof(int), d_off, d_word, v->d_word_weight, P, d_cnt, d_bw, d_bv);
    CS_HIP(ctx, hipGetLastError());
    CS_TRY(cs_d2h(ctx, word, d_word, (size_t)n)); CS_TRY(cs_d2h(ctx, node, d_node, (size_t)n)); CS_TRY(cs_d2h(ctx, bow_count, d_cnt, (size_t)n_frames));
    CS_TRY(cs_d2h(ctx, bow_word, d_bw, (size_t)n)); CS_TRY(cs_d2h(ctx, bow_value, d_bv, (size_t)n));
    return sc.drain();
}

int cs_bow_transform(cs_ctx *ctx, const cs_bow_vocab *v, int n_frames, const int *offsets, const uint8_t *desc, int *word, int *node, int *bow_count, int *bow_word,
                     double *bow_value) {
    if (!ctx || !v || n_frames < 0 || !offsets || !word || !node || !bow_count || !bow_word || !bow_value) return CS_ERR_BAD_ARG;
    if (offsets[0] != 0) { ctx->err = "cs_bow_transform: offsets[0] must be 0"; return CS_ERR_BAD_ARG; }
    int max_n = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (offsets[f + 1] < offsets[f]) { ctx->err = "cs_bow_transform: offsets decrease"; return CS_ERR_BAD_ARG; }
        max_n = std::max(max_n, offsets[f + 1] - offsets[f]);
    }
    if (max_n > BOW_MAX_FRAME) { ctx->err = "cs_bow_transform: more than 8192 features in one frame"; return CS_ERR_CAPACITY; }
    const long n = offsets[n_frames];
    if (n_frames == 0) return CS_OK;
    if (n > 0 && !desc) return CS_ERR_BAD_ARG;
    const int r = bow_transform_dev(ctx, v, n_frames, offsets, desc, max_n, n, word, node, bow_count, bow_word, bow_value);
    ctx->flush();
    return r;
}

static int bow_score_dev(cs_ctx *ctx, int n_vec, const int *off, const int *word, const double *value, int n_pairs, const int *pair_a, const int *pair_b, double *score) {
    const size_t nw = (size_t)off[n_vec];
    cs_scratch sc(ctx);
    int *d_off = nullptr, *d_word = nullptr, *d_pa = nullptr, *d_pb = nullptr;
    double *d_value = nullptr, *d_score = nullptr;
    CS_TRY(sc.alloc(ctx, &d_off, (size_t)n_vec + 1)); CS_TRY(sc.alloc(ctx, &d_word, nw)); CS_TRY(sc.alloc(ctx, &d_value, nw));
    CS_TRY(sc.alloc(ctx, &d_pa, (size_t)n_pairs)); CS_TRY(sc.alloc(ctx, &d_pb, (size_t)n_pairs)); CS_TRY(sc.alloc(ctx, &d_score, (size_t)n_pairs));
    CS_TRY(cs_h2d(ctx, d_off, off, (size_t)n_vec + 1)); CS_TRY(cs_h2d(ctx, d_word, word, nw)); CS_TRY(cs_h2d(ctx, d_value, value, nw));
    CS_TRY(cs_h2d(ctx, d_pa, pair_a, (size_t)n_pairs)); CS_TRY(cs_h2d(ctx, d_pb, pair_b, (size_t)n_pairs));
    CS_LAUNCH(ctx, "bow_score_pairs", bow_score_pairs, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, d_off, d_word, d_value, n_pairs, d_pa, d_pb, d_score);
    CS_HIP(ctx, hipGetLastError());
    CS_TRY(cs_d2h(ctx, score, d_score, (size_t)n_pairs));
    return sc.drain();
}

int cs_bow_score(cs_ctx *ctx, int n_vec, const int *off, const int *word, const double *value, int n_pairs, const int *pair_a, const int *pair_b, double *score) {
    if (!ctx || n_vec < 0 || n_pairs < 0 || !off) return CS_ERR_BAD_ARG;
    if (n_pairs == 0) return CS_OK;
    if (!pair_a || !pair_b || !score || (off[n_vec] > 0 && (!word || !value)) || !csr_ok(n_vec, off, word)) { ctx->err = "cs_bow_score: null array or unsorted vector"; return CS_ERR_BAD_ARG; }
    for (int p = 0; p < n_pairs; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= n_vec || pair_b[p] < 0 || pair_b[p] >= n_vec) { ctx->err = "cs_bow_score: pair index outside the vectors"; return CS_ERR_BAD_ARG; }
    const int r = bow_score_dev(ctx, n_vec, off, word, value, n_pairs, pair_a, pair_b, score);
    ctx->flush();
    return r;
}

int cs_bow_db_create(cs_ctx *ctx, cs_bow_db **out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return CS_ERR_BAD_ARG;
    cs_bow_db *db = new cs_bow_db;
    db->ctx = ctx;
    *out = db;
    return CS_OK;
}

void cs_bow_db_destroy(cs_bow_db *db) {
    if (!db) return;
    db->own.free_all(db->ctx);
    delete db;
}

// The pool only grows at its end.  When it is full, the live vectors are copied one behind the other into a new pool (twice what they and the newcomer need), which
// also drops what erased key frames left behind.
static int bow_db_reserve(cs_ctx *ctx, cs_bow_db *db, long extra) {
    if (db->used + extra <= db->cap) return CS_OK;
    long need = extra;
    for (const auto &e : db->live) need += e.cnt;
    const long cap = std::max(2 * need, 1L << 16);
    int *nw = nullptr;
    double *nv = nullptr;
    CS_TRY(db->own.alloc(ctx, &nw, (size_t)cap));
    if (db->own.alloc(ctx, &nv, (size_t)cap) != CS_OK) { db->own.free_one(ctx, nw); ctx->err = "cs_bow_db_add: out of device memory"; return CS_ERR_NOMEM; }
    long at = 0;
    hipError_t e = hipSuccess;
    for (auto &en : db->live) {
        if (en.cnt > 0 && e == hipSuccess) e = hipMemcpyAsync(nw + at, db->d_word + en.off, (size_t)en.cnt * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream);
        if (en.cnt > 0 && e == hipSuccess) e = hipMemcpyAsync(nv + at, db->d_value + en.off, (size_t)en.cnt * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        en.off = at;
        at += en.cnt;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    db->own.free_one(ctx, db->d_word); // (the copies out of the old pair have drained)
    db->own.free_one(ctx, db->d_value);
    db->d_word = nw; db->d_value = nv; db->cap = cap; db->used = at; db->dead = 0;
    CS_HIP(ctx, e);
    return CS_OK;
}

int cs_bow_db_add(cs_ctx *ctx, cs_bow_db *db, long id, int n, const int *word, const double *value) {
    if (!ctx || !db || n < 0 || (n > 0 && (!word || !value))) return CS_ERR_BAD_ARG;
    const int off2[2] = {0, n};
    if (!csr_ok(1, off2, word)) { ctx->err = "cs_bow_db_add: the words of a BowVector are strictly ascending"; return CS_ERR_BAD_ARG; }
    for (const auto &e : db->live)
        if (e.id == id) { ctx->err = "cs_bow_db_add: the key frame is already in the database"; return CS_ERR_BAD_ARG; }
    const int r = bow_db_reserve(ctx, db, n);
    if (r != CS_OK) return r;
    if (n > 0) {
        CS_HIP(ctx, hipMemcpyAsync(db->d_word + db->used, word, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        CS_HIP(ctx, hipMemcpyAsync(db->d_value + db->used, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's arrays may go
    }
    db->live.push_back({id, db->next_seq++, db->used, n});
    db->used += n;
    return CS_OK;
}

int cs_bow_db_erase(cs_bow_db *db, long id) {
    if (!db) return CS_ERR_BAD_ARG;
    for (size_t i = 0; i < db->live.size(); ++i)
        if (db->live[i].id == id) {
            db->dead += db->live[i].cnt;
            db->live.erase(db->live.begin() + (long)i);
            return CS_OK;
        }
    return CS_OK; // KeyFrameDatabase::erase of a key frame that is in no list changes nothing
}

int cs_bow_db_clear(cs_bow_db *db) {
    if (!db) return CS_ERR_BAD_ARG;
    db->live.clear();
    db->used = 0; db->dead = 0;
    return CS_OK;
}

int cs_bow_db_size(const cs_bow_db *db, int *n_keyframes) {
    if (!db || !n_keyframes) return CS_ERR_BAD_ARG;
    *n_keyframes = (int)db->live.size();
    return CS_OK;
}

// the device part of cs_bow_db_query: common words, smallest common word and score of every (query, key frame) pair into the host arrays
static int bow_query_dev(cs_ctx *ctx, const cs_bow_db *db, int n_query, const int *q_off, const int *q_word, const double *q_value, const long *h_off, const int *h_cnt, int *h_common,
                         int *h_min, double *h_score) {
    const int nk = (int)db->live.size();
    const size_t nw = (size_t)q_off[n_query], np = (size_t)n_query * nk;
    cs_scratch sc(ctx);
    int *d_qoff = nullptr, *d_qw = nullptr, *d_cnt = nullptr, *d_common = nullptr, *d_min = nullptr;
    long *d_off = nullptr;
    double *d_qv = nullptr, *d_score = nullptr;
    CS_TRY(sc.alloc(ctx, &d_qoff, (size_t)n_query + 1)); CS_TRY(sc.alloc(ctx, &d_qw, nw)); CS_TRY(sc.alloc(ctx, &d_qv, nw)); CS_TRY(sc.alloc(ctx, &d_off, (size_t)nk));
    CS_TRY(sc.alloc(ctx, &d_cnt, (size_t)nk)); CS_TRY(sc.alloc(ctx, &d_common, np)); CS_TRY(sc.alloc(ctx, &d_min, np)); CS_TRY(sc.alloc(ctx, &d_score, np));
    CS_TRY(cs_h2d(ctx, d_qoff, q_off, (size_t)n_query + 1)); CS_TRY(cs_h2d(ctx, d_qw, q_word, nw)); CS_TRY(cs_h2d(ctx, d_qv, q_value, nw));
    CS_TRY(cs_h2d(ctx, d_off, h_off, (size_t)nk)); CS_TRY(cs_h2d(ctx, d_cnt, h_cnt, (size_t)nk));
    CS_LAUNCH(ctx, "bow_query", bow_query, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, n_query, d_qoff, d_qw, d_qv, nk, d_off, d_cnt, db->d_word, db->d_value, d_common, d_min,
              d_score);
    CS_HIP(ctx, hipGetLastError());
    CS_TRY(cs_d2h(ctx, h_common, d_common, np)); CS_TRY(cs_d2h(ctx, h_min, d_min, np)); CS_TRY(cs_d2h(ctx, h_score, d_score, np));
    return sc.drain();
}

int cs_bow_db_query(cs_ctx *ctx, cs_bow_db *db, int n_query, const int *q_off, const int *q_word, const double *q_value, long cap, long *n_out, int *out_query, long *out_id,
                    long *out_order, int *out_common, int *out_minword, double *out_score) {
    if (!ctx || !db || n_query < 0 || !q_off || !n_out || cap < 0) return CS_ERR_BAD_ARG;
    *n_out = 0;
    const int nk = (int)db->live.size();
    if (n_query == 0 || nk == 0) return CS_OK;
    if ((q_off[n_query] > 0 && (!q_word || !q_value)) || !csr_ok(n_query, q_off, q_word)) { ctx->err = "cs_bow_db_query: null array or unsorted query vector"; return CS_ERR_BAD_ARG; }
    if (cap > 0 && (!out_query || !out_id || !out_order || !out_common || !out_minword || !out_score)) return CS_ERR_BAD_ARG;
    const size_t np = (size_t)n_query * nk;
    std::vector<long> h_off(nk);
    std::vector<int> h_cnt(nk);
    for (int i = 0; i < nk; ++i) { h_off[i] = db->live[i].off; h_cnt[i] = db->live[i].cnt; }
    std::vector<int> h_common(np), h_min(np);
    std::vector<double> h_score(np);
    const int r = bow_query_dev(ctx, db, n_query, q_off, q_word, q_value, h_off.data(), h_cnt.data(), h_common.data(), h_min.data(), h_score.data());
    ctx->flush();
    if (r != CS_OK) return r;
    long m = 0;
    for (size_t p = 0; p < np; ++p) {
        if (h_common[p] <= 0) continue;
        if (m < cap) {
            const auto &e = db->live[p % nk];
            out_query[m] = (int)(p / nk); out_id[m] = e.id; out_order[m] = e.seq; out_common[m] = h_common[p]; out_minword[m] = h_min[p]; out_score[m] = h_score[p];
        }
        ++m;
    }
    *n_out = m;
    if (m > cap) { ctx->err = "cs_bow_db_query: more pairs than the output arrays hold"; return CS_ERR_CAPACITY; }
    return CS_OK;
}

} // extern "C"
