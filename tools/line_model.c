/* line_model.c -- CPU model of the compact records' 128-B line traffic under three record orders
 * (analysis tool, tools/line_model.py).
 *
 * visit_seq replays the Bvh2 closest-hit traversal (the loop of tools/trav_sim.c, the oracle's
 * node order) and writes each ray's visit sequence.  layout gives every node its byte offset in
 * the compact copy (internal 32 B, leaf 48 B) for
 *   0  depth-first: the 64-B tree's order, packed back to back (the left child is the next record);
 *   1  sibling pairs: the two children of a node side by side in one line, pairs depth-first;
 *   2  treelets: a node and both its children in one line; the grandchildren start treelets of
 *      their own, a sibling pair of treelets side by side (in one line where they fit), pairs of
 *      treelets depth-first.  Orders 1 and 2 are mcrt_qnodes.hip qnode_order_offsets, restated.
 * lru_misses pushes the records' lines through one CU's L1: a fully associative LRU of `lines`
 * 128-B lines shared by `slots` resident waves.  Interleaving assumption: the resident waves take
 * turns, one loop step each (a step = the k-th visit of every lane still walking, as the
 * lock-step wave does); a wave that ends hands its slot to the next wave of the CU's contiguous
 * run of the queue.
 * Build: gcc -O2 -shared -fPIC tools/line_model.c -o line_model.so -lm
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float lmin[3]; uint32_t left; float lmax[3]; uint32_t mesh; float rmin[3]; uint32_t right; float rmax[3]; uint32_t prim; } Node;
typedef struct { float o[4]; float d[4]; int32_t extra[2]; int32_t bf; int32_t pad; } Ray;
#define INV 0xffffffffu

static inline float sinv(float d) { return 1.0f / (fabsf(d) > 1e-8f ? d : copysignf(1e-8f, d)); }
static void bbox(const float* lo, const float* hi, const float* inv, const float* oxi, float tmax, float* t0, float* t1) {
    float f[3], n[3];
    for (int k = 0; k < 3; ++k) { f[k] = fmaf(hi[k], inv[k], oxi[k]); n[k] = fmaf(lo[k], inv[k], oxi[k]); }
    *t1 = fminf(fminf(fminf(fmaxf(f[0], n[0]), fmaxf(f[1], n[1])), fmaxf(f[2], n[2])), tmax);
    *t0 = fmaxf(fmaxf(fmaxf(fminf(f[0], n[0]), fminf(f[1], n[1])), fminf(f[2], n[2])), 0.f);
}
static float tri(const Ray* r, const Node* n, float tmax) {
    float e1[3], e2[3], s1[3], d[3], s2[3];
    for (int k = 0; k < 3; ++k) { e1[k] = n->lmax[k] - n->lmin[k]; e2[k] = n->rmin[k] - n->lmin[k]; }
    s1[0] = r->d[1] * e2[2] - r->d[2] * e2[1]; s1[1] = r->d[2] * e2[0] - r->d[0] * e2[2]; s1[2] = r->d[0] * e2[1] - r->d[1] * e2[0];
    float den = s1[0] * e1[0] + s1[1] * e1[1] + s1[2] * e1[2];
    if (den == 0.f) return tmax;
    float id = 1.0f / den;
    for (int k = 0; k < 3; ++k) d[k] = r->o[k] - n->lmin[k];
    float b1 = (d[0] * s1[0] + d[1] * s1[1] + d[2] * s1[2]) * id;
    s2[0] = d[1] * e1[2] - d[2] * e1[1]; s2[1] = d[2] * e1[0] - d[0] * e1[2]; s2[2] = d[0] * e1[1] - d[1] * e1[0];
    float b2 = (r->d[0] * s2[0] + r->d[1] * s2[1] + r->d[2] * s2[2]) * id;
    float t = (e2[0] * s2[0] + e2[1] * s2[1] + e2[2] * s2[2]) * id;
    if (b1 < 0.f || b1 > 1.f || b2 < 0.f || b1 + b2 > 1.f || t < 0.f || t > tmax) return tmax;
    return t;
}

/* Closest-hit walks of n rays: ray i's visits are seq[start[i] .. start[i + 1]) (node indices).
 * Returns the total number of visits; with seq == NULL it only counts (first pass). */
int64_t visit_seq(const Node* nodes, const Ray* rays, int n, uint32_t* seq, int64_t* start, float* hit_t, int32_t* hit_node) {
    static uint32_t stack[1 << 16];
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) {
        const Ray* r = &rays[i];
        start[i] = tot;
        hit_t[i] = -1;
        hit_node[i] = -1;
        if (r->extra[1] == 0) continue;
        float inv[3], oxi[3];
        for (int k = 0; k < 3; ++k) { inv[k] = sinv(r->d[k]); oxi[k] = -r->o[k] * inv[k]; }
        float ct = r->o[3];
        uint32_t addr = 0, best = INV;
        int sp = 0;
        stack[sp++] = INV;
        while (addr != INV) {
            const Node* nd = &nodes[addr];
            if (seq) seq[tot] = addr;
            ++tot;
            if (nd->left != INV) {
                float a0, a1, b0, b1;
                bbox(nd->lmin, nd->lmax, inv, oxi, ct, &a0, &a1);
                bbox(nd->rmin, nd->rmax, inv, oxi, ct, &b0, &b1);
                int h0 = a0 <= a1, h1 = b0 <= b1, c1 = h1 && (a0 > b0);
                if (h0 || h1) {
                    uint32_t def;
                    if (c1 || !h0) { addr = nd->right; def = nd->left; } else { addr = nd->left; def = nd->right; }
                    if (h0 && h1) stack[sp++] = def;
                    continue;
                }
            } else if (r->extra[0] != (int)nd->mesh) {
                float t = tri(r, nd, ct);
                if (t < ct) { ct = t; best = addr; }
            }
            addr = stack[--sp];
        }
        hit_t[i] = ct;
        hit_node[i] = best == INV ? -1 : (int32_t)best;
    }
    start[n] = tot;
    return tot;
}

static inline int isleaf(const Node* nodes, uint32_t i) { return nodes[i].left == INV; }
static inline uint32_t rsize(const Node* nodes, uint32_t i) { return isleaf(nodes, i) ? 48u : 32u; }
/* the next free offset at which `bytes` do not cross a line */
static inline uint64_t fit(uint64_t cur, uint32_t bytes) { return (cur & 127u) + bytes > 128u ? (cur + 127u) & ~(uint64_t)127u : cur; }
static uint32_t treelet_bytes(const Node* nodes, uint32_t g) {
    return isleaf(nodes, g) ? 48u : 32u + rsize(nodes, nodes[g].left) + rsize(nodes, nodes[g].right);
}

/* off[i] = byte offset of node i's compact record; returns the copy's size.  Parents come before
 * their children in the node numbering (checked: a child index above its parent's). */
uint64_t layout(const Node* nodes, uint32_t n, int order, uint64_t* off) {
    uint64_t cur = 0;
    if (order == 0) {
        for (uint32_t i = 0; i < n; ++i) { off[i] = cur; cur += rsize(nodes, i); }
        return cur;
    }
    /* explicit stack of (node, role): role 0 = starts a treelet / a pair's parent for order 1 */
    uint32_t* stk = (uint32_t*)malloc(sizeof(uint32_t) * 8 * 4096);
    int sp = 0;
    off[0] = 0;
    cur = rsize(nodes, 0);
    if (order == 1) {
        stk[sp++] = 0;
        while (sp) {
            const uint32_t p = stk[--sp];
            if (isleaf(nodes, p)) continue;
            const uint32_t l = nodes[p].left, r = nodes[p].right;
            cur = fit(cur, rsize(nodes, l) + rsize(nodes, r));
            off[l] = cur; cur += rsize(nodes, l);
            off[r] = cur; cur += rsize(nodes, r);
            stk[sp++] = r;   /* the left subtree's pairs first */
            stk[sp++] = l;
        }
        free(stk);
        return cur;
    }
    /* order 2: the root's treelet, then for every member child c of a treelet (in depth-first
     * order) the pair of treelets its children start */
    if (!isleaf(nodes, 0)) {
        const uint32_t l = nodes[0].left, r = nodes[0].right;
        off[l] = cur; cur += rsize(nodes, l);
        off[r] = cur; cur += rsize(nodes, r);
        stk[sp++] = r;
        stk[sp++] = l;
    }
    while (sp) {
        const uint32_t c = stk[--sp];   /* a treelet's child member: its children start treelets */
        if (isleaf(nodes, c)) continue;
        const uint32_t g[2] = {nodes[c].left, nodes[c].right};
        for (int k = 0; k < 2; ++k) {
            cur = fit(cur, treelet_bytes(nodes, g[k]));
            off[g[k]] = cur; cur += rsize(nodes, g[k]);
            if (!isleaf(nodes, g[k])) {
                const uint32_t l = nodes[g[k]].left, r = nodes[g[k]].right;
                off[l] = cur; cur += rsize(nodes, l);
                off[r] = cur; cur += rsize(nodes, r);
            }
        }
        for (int k = 1; k >= 0; --k)
            if (!isleaf(nodes, g[k])) { stk[sp++] = nodes[g[k]].right; stk[sp++] = nodes[g[k]].left; }
    }
    free(stk);
    return cur;
}

/* One CU: waves [w0, w1) of 64 consecutive rays each, `slots` resident at a time, an LRU of `lines`
 * lines over a copy of `bytes` bytes.  out[0] += record visits, out[1] += line misses, out[2] +=
 * line accesses (a record that crosses a line boundary accesses two), out[3] += wave steps. */
void lru_misses(const Node* nodes, const uint64_t* off, uint64_t bytes, const uint32_t* seq, const int64_t* start, int nrays,
                int w0, int w1, int slots, int lines, int64_t* out) {
    const uint64_t nl = (bytes + 127) / 128 + 1;
    int32_t* where = (int32_t*)malloc(sizeof(int32_t) * nl);   /* line -> way, or -1 */
    memset(where, 0xff, sizeof(int32_t) * nl);
    uint64_t* held = (uint64_t*)malloc(sizeof(uint64_t) * lines);
    int* prev = (int*)malloc(sizeof(int) * lines);
    int* nxt = (int*)malloc(sizeof(int) * lines);
    int head = -1, tail = -1, used = 0;   /* head = most recent */
    int* wave = (int*)malloc(sizeof(int) * slots);
    int64_t* step = (int64_t*)malloc(sizeof(int64_t) * slots);
    int next = w0, live = 0;
    for (int s = 0; s < slots; ++s) { wave[s] = next < w1 ? next++ : -1; step[s] = 0; live += wave[s] >= 0; }
    while (live) {
        for (int s = 0; s < slots; ++s) {
            if (wave[s] < 0) continue;
            int any = 0;
            for (int l = 0; l < 64; ++l) {
                const int ray = wave[s] * 64 + l;
                if (ray >= nrays) break;
                const int64_t j = start[ray] + step[s];
                if (j >= start[ray + 1]) continue;
                any = 1;
                const uint32_t node = seq[j];
                const uint64_t a = off[node], b = a + (nodes[node].left == INV ? 48u : 32u) - 1;
                out[0] += 1;
                for (uint64_t ln = a >> 7; ln <= b >> 7; ++ln) {
                    out[2] += 1;
                    int w = where[ln];
                    if (w < 0) {
                        out[1] += 1;
                        if (used < lines) {
                            w = used++;
                        } else {   /* evict the least recent */
                            w = tail;
                            where[held[w]] = -1;
                            tail = prev[w];
                            if (tail >= 0) nxt[tail] = -1; else head = -1;
                        }
                        held[w] = ln;
                        where[ln] = w;
                    } else {   /* unlink */
                        if (w == head) continue;
                        if (prev[w] >= 0) nxt[prev[w]] = nxt[w];
                        if (nxt[w] >= 0) prev[nxt[w]] = prev[w]; else tail = prev[w];
                    }
                    prev[w] = -1;
                    nxt[w] = head;
                    if (head >= 0) prev[head] = w; else tail = w;
                    head = w;
                }
            }
            if (any) {
                out[3] += 1;
                ++step[s];
            } else {
                wave[s] = next < w1 ? next++ : -1;
                step[s] = 0;
                if (wave[s] < 0) --live;
            }
        }
    }
    free(where); free(held); free(prev); free(nxt); free(wave); free(step);
}
