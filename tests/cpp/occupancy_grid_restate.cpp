// CPU restatement of OccupancyGridMap (algorithms/mapping/occupancy_grid_map.hpp:27-190, 417-472, 482-1687 of the reference, without
// extract_visible_points) as this project specifies it: single-threaded, every sum in input order, rays in input
// order, slots claimed in that order. Compiled by the tests that use it with -ffp-contract=off.
//
// Where it departs from the reference it does so with the device, on purpose:
//   * the ray walk is the BOUNDED walk: exactly |dix| + |diy| + |diz| steps, an axis that has reached the target's cell no longer
//     competes (the reference loops until it lands on the target cell, :880-899). This walk is the specification;
//   * a ray that ends at a non-finite point or outside the 21-bit cell range, or is shorter than sqrt(FLT_EPSILON), posts nothing;
//     a frame whose sensor lies outside the range carves nothing;
//   * pending log-odds are two counts per voxel, applied as hits * log_hit + misses * log_miss;
//   * the growth before the walk goes to its last capacity in one rehash; a pruned slot's covariance sums are cleared.
// The log-Euclidean covariance maps, the key and the point transform are the oracle's (oracle/oracle_voxel_hash_map.hpp).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../oracle/oracle_voxel_hash_map.hpp"

namespace {

using oracle::Mat3;

constexpr uint64_t kInvalid = ~0ull, kDeleted = ~0ull - 1;
constexpr size_t kMaxProbe = 128;  // :1679
constexpr size_t kNoSlot = ~(size_t)0;
constexpr int kOffset = 1 << 20, kMask = (1 << 21) - 1;
constexpr size_t kLadder[11] = {30029, 60013, 120011, 240007, 480013, 960017, 1920001, 3840007, 7680017, 15360013, 30720007};

struct Core { float sx = 0, sy = 0, sz = 0, log_odds = 0; uint32_t hits = 0, misses = 0, hits_applied = 0, misses_applied = 0; };
struct Cov { float v[6] = {0, 0, 0, 0, 0, 0}; };
struct Color { float v[4] = {0, 0, 0, 0}; };

uint64_t cell_key(int x, int y, int z) {  // grid_to_key_device (:903-920)
    const int cx = x + kOffset, cy = y + kOffset, cz = z + kOffset;
    if (cx < 0 || cx > kMask || cy < 0 || cy > kMask || cz < 0 || cz > kMask) return kInvalid;
    return (uint64_t)cx | ((uint64_t)cy << 21) | ((uint64_t)cz << 42);
}

// The bounded walk over traverse_ray_exclusive_impl's arithmetic (:823-900). visit(ix, iy, iz) is called for every cell stepped
// into, the last one (the target's) included; returns the number of steps = |dix| + |diy| + |diz|.
template <class Visit>
uint64_t bounded_walk(float ox, float oy, float oz, float wx, float wy, float wz, float inv, Visit&& visit) {
    const float sox = ox * inv, soy = oy * inv, soz = oz * inv;
    const float fox = std::floor(sox), foy = std::floor(soy), foz = std::floor(soz);
    int ix = (int)fox, iy = (int)foy, iz = (int)foz;
    const float stx = wx * inv, sty = wy * inv, stz = wz * inv;
    const int tx = (int)std::floor(stx), ty = (int)std::floor(sty), tz = (int)std::floor(stz);
    const uint64_t steps = (uint64_t)std::abs(tx - ix) + (uint64_t)std::abs(ty - iy) + (uint64_t)std::abs(tz - iz);
    if (steps == 0) return 0;
    const float dir_x = stx - sox, dir_y = sty - soy, dir_z = stz - soz;
    const float ax = std::fabs(dir_x), ay = std::fabs(dir_y), az = std::fabs(dir_z);
    const int step_x = (dir_x > 0.0f) ? 1 : ((dir_x < 0.0f) ? -1 : 0);
    const int step_y = (dir_y > 0.0f) ? 1 : ((dir_y < 0.0f) ? -1 : 0);
    const int step_z = (dir_z > 0.0f) ? 1 : ((dir_z < 0.0f) ? -1 : 0);
    const float frac_x = sox - fox, frac_y = soy - foy, frac_z = soz - foz;
    const float inf = INFINITY;
    const float inv_x = (ax > FLT_EPSILON) ? (1.0f / ax) : inf;
    const float inv_y = (ay > FLT_EPSILON) ? (1.0f / ay) : inf;
    const float inv_z = (az > FLT_EPSILON) ? (1.0f / az) : inf;
    float t_max_x = (step_x != 0) ? ((step_x > 0 ? (1.0f - frac_x) : frac_x) * inv_x) : inf;
    float t_max_y = (step_y != 0) ? ((step_y > 0 ? (1.0f - frac_y) : frac_y) * inv_y) : inf;
    float t_max_z = (step_z != 0) ? ((step_z > 0 ? (1.0f - frac_z) : frac_z) * inv_z) : inf;
    const float t_delta_x = (step_x != 0) ? inv_x : inf;
    const float t_delta_y = (step_y != 0) ? inv_y : inf;
    const float t_delta_z = (step_z != 0) ? inv_z : inf;
    for (uint64_t s = 1; s <= steps; ++s) {
        const bool ux = ix != tx, uy = iy != ty, uz = iz != tz;
        int axis;
        if (ux && (!uy || t_max_x <= t_max_y) && (!uz || t_max_x <= t_max_z)) axis = 0;
        else if (uy && (!uz || t_max_y <= t_max_z)) axis = 1;
        else if (uz) axis = 2;
        else axis = uy ? 1 : 0;
        if (axis == 0) { ix += step_x; t_max_x += t_delta_x; }
        else if (axis == 1) { iy += step_y; t_max_y += t_delta_y; }
        else { iz += step_z; t_max_z += t_delta_z; }
        visit(ix, iy, iz);
    }
    return steps;
}

struct Map {
    float voxel_size = 0.1f, inv = 10.0f;
    float log_hit = 0.85f, log_miss = -0.4f, lo_min = -4.0f, lo_max = 4.0f, occ_prob = 0.5f, occ_thr = 0.0f;
    bool free_space = true, pruning = true, has_cov = false, has_rgb = false, has_intensity = false;
    uint32_t frame = 0, stale = 100;
    float rehash_threshold = 0.7f;
    size_t capacity = kLadder[0], voxel_num = 0;
    std::vector<uint64_t> key;
    std::vector<Core> core;
    std::vector<Cov> cov;
    std::vector<Color> color;
    std::vector<float> intensity;
    std::vector<uint32_t> last;

    void allocate(size_t cap) {
        key.assign(cap, kInvalid); core.assign(cap, Core{}); cov.assign(cap, Cov{}); color.assign(cap, Color{});
        intensity.assign(cap, 0.0f); last.assign(cap, 0u);
        capacity = cap;
    }
    void clear() {  // :42-69
        voxel_num = 0; has_cov = has_rgb = has_intensity = false; frame = 0;
        allocate(kLadder[0]);
    }
    static size_t slot_id(uint64_t h, size_t probe, size_t cap) { return (size_t)((h + probe * ((cap - 2) - (h % (cap - 2)))) % cap); }
    static bool live(uint64_t k) { return k != kInvalid && k != kDeleted; }
    size_t next_capacity(size_t cap) const {
        for (const size_t c : kLadder)
            if (c > cap) return c;
        return cap;
    }
    size_t find_or_claim(uint64_t h) {  // global_reduction's slot search (:795-818), one arrival at a time
        for (size_t p = 0; p < kMaxProbe; ++p) {
            const size_t s = slot_id(h, p, capacity);
            if (key[s] == kInvalid || key[s] == kDeleted) { key[s] = h; ++voxel_num; return s; }
            if (key[s] == h) return s;
        }
        return kNoSlot;
    }
    size_t find(uint64_t h) const {  // :591-609
        for (size_t p = 0; p < kMaxProbe; ++p) {
            const size_t s = slot_id(h, p, capacity);
            if (key[s] == h) return s;
            if (key[s] == kInvalid) return kNoSlot;
        }
        return kNoSlot;
    }
    void rehash(size_t new_cap) {  // :652-782, slot order
        if (capacity >= new_cap) return;
        const auto okey = key; const auto ocore = core; const auto ocov = cov; const auto ocol = color;
        const auto oint = intensity; const auto olast = last;
        allocate(new_cap);
        size_t num = 0;
        for (size_t i = 0; i < okey.size(); ++i) {
            if (!live(okey[i])) continue;
            for (size_t p = 0; p < kMaxProbe; ++p) {
                const size_t s = slot_id(okey[i], p, capacity);
                if (key[s] != kInvalid) continue;
                key[s] = okey[i]; core[s] = ocore[i]; last[s] = olast[i];
                if (has_cov) cov[s] = ocov[i];
                if (has_rgb) color[s] = ocol[i];
                if (has_intensity) intensity[s] = oint[i];
                ++num;
                break;
            }
        }
        voxel_num = num;
    }
    static void world_point(const float* p, const float* T, float* w) {
        const float q[4] = {p[0], p[1], p[2], 1.0f};
        oracle::transform_point(q, w, T);
    }
    // rotate_covariance_upper_triangle (:994-1028) + encode_covariance_for_aggregation (:1030-1049)
    static Cov encode_cov(const float* c16, const float* T) {
        const float cxx = c16[0], cxy = c16[4], cxz = c16[8], cyy = c16[5], cyz = c16[9], czz = c16[10];
        const float r00 = T[0], r01 = T[4], r02 = T[8], r10 = T[1], r11 = T[5], r12 = T[9], r20 = T[2], r21 = T[6], r22 = T[10];
        auto f3 = [](float a, float b, float c, float d, float e, float f) { return std::fmaf(a, b, std::fmaf(c, d, e * f)); };
        const float a00 = f3(r02, cxz, r01, cxy, r00, cxx), a01 = f3(r02, cyz, r01, cyy, r00, cxy), a02 = f3(r02, czz, r01, cyz, r00, cxz);
        const float a10 = f3(r12, cxz, r11, cxy, r10, cxx), a11 = f3(r12, cyz, r11, cyy, r10, cxy), a12 = f3(r12, czz, r11, cyz, r10, cxz);
        const float a20 = f3(r22, cxz, r21, cxy, r20, cxx), a21 = f3(r22, cyz, r21, cyy, r20, cxy), a22 = f3(r22, czz, r21, cyz, r20, cxz);
        Mat3 m;
        m(0, 0) = f3(a02, r02, a01, r01, a00, r00);
        m(0, 1) = m(1, 0) = f3(a02, r12, a01, r11, a00, r10);
        m(0, 2) = m(2, 0) = f3(a02, r22, a01, r21, a00, r20);
        m(1, 1) = f3(a12, r12, a11, r11, a10, r10);
        m(1, 2) = m(2, 1) = f3(a12, r22, a11, r21, a10, r20);
        m(2, 2) = f3(a22, r22, a21, r21, a20, r20);
        const Mat3 l = oracle::log_spd_3x3(m);
        Cov o;
        o.v[0] = l(0, 0); o.v[1] = l(0, 1); o.v[2] = l(0, 2); o.v[3] = l(1, 1); o.v[4] = l(1, 2); o.v[5] = l(2, 2);
        return o;
    }
    void hits(const float* pts, const float* covs, const float* rgb, const float* inten, size_t n, const float* T) {  // :1072-1233
        for (size_t i = 0; i < n; ++i) {
            float w[4];
            world_point(pts + 4 * i, T, w);
            const uint64_t h = oracle::compute_voxel_bit(w, inv);
            if (h == kInvalid) continue;
            const size_t s = find_or_claim(h);
            if (s == kNoSlot) continue;
            core[s].sx += w[0]; core[s].sy += w[1]; core[s].sz += w[2]; core[s].hits += 1;
            if (covs) {
                const Cov c = encode_cov(covs + 16 * i, T);
                for (int k = 0; k < 6; ++k) cov[s].v[k] += c.v[k];
            }
            if (rgb) for (int k = 0; k < 4; ++k) color[s].v[k] += rgb[4 * i + k];
            if (inten) intensity[s] += inten[i];
            last[s] = frame;
        }
    }
    struct Ray { float w[4]; bool cast; };
    Ray make_ray(const float* p, const float* T, float ox, float oy, float oz) const {
        Ray r;
        world_point(p, T, r.w);
        r.cast = false;
        if (oracle::compute_voxel_bit(r.w, inv) == kInvalid) return r;
        const float dx = r.w[0] - ox, dy = r.w[1] - oy, dz = r.w[2] - oz;
        const float dist_sq = dx * dx + dy * dy + dz * dz;
        if (dist_sq <= FLT_EPSILON) return r;
        r.cast = true;
        return r;
    }
    void post_miss(uint64_t k) {
        const size_t s = find_or_claim(k);
        if (s == kNoSlot) return;
        core[s].misses += 1;
        last[s] = frame;
    }
    void carve(const float* pts, size_t n, const float* T) {  // :1235-1455
        const float ox = T[12], oy = T[13], oz = T[14];
        const float fx = std::floor(ox * inv), fy = std::floor(oy * inv), fz = std::floor(oz * inv);
        const float lim = (float)kOffset;
        if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) return;
        const int oix = (int)fx, oiy = (int)fy, oiz = (int)fz;
        const uint64_t origin_key = cell_key(oix, oiy, oiz);
        bool origin_hit = false;
        uint64_t expected = 0;
        for (size_t i = 0; i < n; ++i) {
            const Ray r = make_ray(pts + 4 * i, T, ox, oy, oz);
            if (oracle::compute_voxel_bit(r.w, inv) == origin_key) origin_hit = true;
            if (!r.cast) continue;
            const uint64_t steps = (uint64_t)std::abs((int)std::floor(r.w[0] * inv) - oix) +
                                   (uint64_t)std::abs((int)std::floor(r.w[1] * inv) - oiy) +
                                   (uint64_t)std::abs((int)std::floor(r.w[2] * inv) - oiz);
            expected += steps > 0 ? steps + 1 : 0;
        }
        if (expected == 0) return;
        const float required = (float)(voxel_num + expected);
        size_t cap = capacity;
        while (rehash_threshold < required / (float)cap) {
            const size_t next = next_capacity(cap);
            if (next <= cap) break;
            cap = next;
        }
        rehash(cap);
        for (size_t i = 0; i < n; ++i) {
            const Ray r = make_ray(pts + 4 * i, T, ox, oy, oz);
            if (!r.cast) continue;
            const int tx = (int)std::floor(r.w[0] * inv), ty = (int)std::floor(r.w[1] * inv), tz = (int)std::floor(r.w[2] * inv);
            if (tx == oix && ty == oiy && tz == oiz) continue;
            if (!origin_hit) post_miss(origin_key);  // :1427-1433
            bounded_walk(ox, oy, oz, r.w[0], r.w[1], r.w[2], inv, [&](int x, int y, int z) {
                if (x == tx && y == ty && z == tz) return;  // the hit cell: the last step, by construction
                const uint64_t k = cell_key(x, y, z);
                if (k != kInvalid) post_miss(k);
            });
        }
    }
    void apply() {  // :1457-1483
        for (size_t i = 0; i < capacity; ++i) {
            if (!live(key[i])) continue;
            Core& c = core[i];
            const uint32_t h = c.hits - c.hits_applied, m = c.misses - c.misses_applied;
            if (h == 0 && m == 0) continue;
            const float delta = (float)h * log_hit + (float)m * log_miss;
            if (delta != 0.0f) c.log_odds = std::fmax(lo_min, std::fmin(lo_max, c.log_odds + delta));
            c.hits_applied = c.hits;
            c.misses_applied = c.misses;
        }
    }
    void prune() {  // :1485-1528
        if (frame < stale) return;
        size_t kept = 0;
        for (size_t i = 0; i < capacity; ++i) {
            if (!live(key[i])) continue;
            if ((frame - last[i]) > stale) {
                key[i] = kDeleted; core[i] = Core{}; cov[i] = Cov{}; color[i] = Color{}; intensity[i] = 0.0f; last[i] = 0;
                continue;
            }
            ++kept;
        }
        voxel_num = kept;
    }
    void add(const float* pts, const float* covs, const float* rgb, const float* inten, size_t n, const float* T) {  // :129-163
        if (n == 0) return;
        if (rehash_threshold < (float)voxel_num / (float)capacity) {
            const size_t next = next_capacity(capacity);
            if (next > capacity) rehash(next);
        }
        has_cov |= covs != nullptr; has_rgb |= rgb != nullptr; has_intensity |= inten != nullptr;
        hits(pts, covs, rgb, inten, n, T);
        if (free_space && log_miss != 0.0f) carve(pts, n, T);
        apply();
        if (pruning) prune();
        ++frame;
    }
};

}  // namespace

extern "C" {

void* ogm_restate_create(float voxel_size) {
    if (!(voxel_size > 0.0f)) return nullptr;  // :74-76
    Map* m = new Map();
    m->voxel_size = voxel_size;
    m->inv = 1.0f / voxel_size;
    m->occ_thr = std::log(0.5f / (1.0f - 0.5f));
    m->clear();
    return m;
}
void ogm_restate_destroy(void* h) { delete static_cast<Map*>(h); }
void ogm_restate_clear(void* h) { static_cast<Map*>(h)->clear(); }

int ogm_restate_set_limits(void* h, float lo, float hi) {  // :107-113; 1 = std::invalid_argument
    Map* m = static_cast<Map*>(h);
    if (lo > hi) return 1;
    m->lo_min = lo; m->lo_max = hi;
    return 0;
}
int ogm_restate_set(void* h, int param, float v) {  // the parameters of SP_OGM_*
    Map* m = static_cast<Map*>(h);
    switch (param) {
        case 0: if (!(v > 0.0f)) return 1; m->voxel_size = v; m->inv = 1.0f / v; return 0;
        case 1: m->log_hit = v; return 0;
        case 2: m->log_miss = v; return 0;
        case 3: return ogm_restate_set_limits(h, v, m->lo_max);
        case 4: return ogm_restate_set_limits(h, m->lo_min, v);
        case 5: if (!(v > 0.0f) || !(v < 1.0f)) return 1; m->occ_prob = v; m->occ_thr = std::log(v / (1.0f - v)); return 0;
        case 6: m->free_space = v != 0.0f; return 0;
        case 7: m->pruning = v != 0.0f; return 0;
        case 8: m->stale = (uint32_t)v; return 0;
        case 9: m->rehash_threshold = v; return 0;
    }
    return 1;
}
float ogm_restate_threshold_log_odds(void* h) { return static_cast<Map*>(h)->occ_thr; }
uint64_t ogm_restate_info(void* h, int what) {  // SP_OGM_INFO_*
    const Map* m = static_cast<Map*>(h);
    switch (what) {
        case 0: return m->voxel_num;
        case 1: return m->capacity;
        case 2: return m->frame;
        case 3: return m->has_cov;
        case 4: return m->has_rgb;
        case 5: return m->has_intensity;
    }
    return 0;
}
void ogm_restate_add(void* h, const float* pts, const float* covs, const float* rgb, const float* inten, uint64_t n,
                     const float* pose16) {
    static_cast<Map*>(h)->add(pts, covs, rgb, inten, (size_t)n, pose16);
}

// :169-181, 1530-1639, slot order. Outputs hold voxel_num rows; attribute outputs are written when the map holds the attribute.
uint64_t ogm_restate_extract(void* h, const float* sensor3, float max_distance, float* pts_out, float* cov_out, float* rgb_out,
                             float* inten_out, uint64_t* keys_out) {
    const Map* m = static_cast<Map*>(h);
    if (m->voxel_num == 0) return 0;
    uint64_t out = 0;
    for (size_t i = 0; i < m->capacity; ++i) {
        if (!Map::live(m->key[i])) continue;
        const Core& c = m->core[i];
        if (c.hits == 0u || c.log_odds < m->occ_thr) continue;
        const float inv = 1.0f / (float)c.hits;
        const float cx = c.sx * inv, cy = c.sy * inv, cz = c.sz * inv;
        const float dx = std::fabs(cx - sensor3[0]), dy = std::fabs(cy - sensor3[1]), dz = std::fabs(cz - sensor3[2]);
        if (std::fmax(std::fmax(dx, dy), dz) > max_distance) continue;
        pts_out[4 * out] = cx; pts_out[4 * out + 1] = cy; pts_out[4 * out + 2] = cz; pts_out[4 * out + 3] = 1.0f;
        if (cov_out && m->has_cov) {  // decode_covariance_average (:1051-1070)
            const float* v = m->cov[i].v;
            Mat3 a;
            a(0, 0) = v[0] * inv; a(0, 1) = a(1, 0) = v[1] * inv; a(0, 2) = a(2, 0) = v[2] * inv;
            a(1, 1) = v[3] * inv; a(1, 2) = a(2, 1) = v[4] * inv; a(2, 2) = v[5] * inv;
            const Mat3 e = oracle::exp_spd_3x3(a);
            float* o = cov_out + 16 * out;
            for (int k = 0; k < 16; ++k) o[k] = 0.0f;
            for (int col = 0; col < 3; ++col)
                for (int row = 0; row < 3; ++row) o[col * 4 + row] = e(row, col);
        }
        if (rgb_out && m->has_rgb) for (int k = 0; k < 4; ++k) rgb_out[4 * out + k] = m->color[i].v[k] * inv;
        if (inten_out && m->has_intensity) inten_out[out] = m->intensity[i] * inv;
        if (keys_out) keys_out[out] = m->key[i];
        ++out;
    }
    return out;
}

float ogm_restate_overlap(void* h, const float* pts, uint64_t n, const float* pose16) {  // :417-472
    const Map* m = static_cast<Map*>(h);
    if (n == 0 || !pts || m->voxel_num == 0) return 0.0f;
    uint32_t hits = 0;
    for (uint64_t i = 0; i < n; ++i) {
        float w[4];
        Map::world_point(pts + 4 * i, pose16, w);
        const uint64_t k = oracle::compute_voxel_bit(w, m->inv);
        if (k == kInvalid) continue;
        const size_t s = m->find(k);
        if (s != kNoSlot && m->core[s].hits > 0u && !(m->core[s].log_odds < m->occ_thr)) ++hits;
    }
    return (float)hits / (float)n;
}

float ogm_restate_probability(void* h, const float* xyz) {  // :85-93
    const Map* m = static_cast<Map*>(h);
    const float w[4] = {xyz[0], xyz[1], xyz[2], 1.0f};
    const uint64_t k = oracle::compute_voxel_bit(w, m->inv);
    if (k == kInvalid) return 0.5f;
    const size_t s = m->find(k);
    if (s == kNoSlot) return 0.5f;
    return 1.0f / (1.0f + std::exp(-m->core[s].log_odds));
}

// every live slot in slot order; outputs hold voxel_num rows (any may be null)
uint64_t ogm_restate_export(void* h, uint64_t* keys, uint32_t* hits, uint32_t* misses, float* log_odds, uint32_t* last, float* xyz,
                            float* cov, float* rgb, float* inten) {
    const Map* m = static_cast<Map*>(h);
    uint64_t o = 0;
    for (size_t i = 0; i < m->capacity; ++i) {
        if (!Map::live(m->key[i])) continue;
        const Core& c = m->core[i];
        if (keys) keys[o] = m->key[i];
        if (hits) hits[o] = c.hits;
        if (misses) misses[o] = c.misses;
        if (log_odds) log_odds[o] = c.log_odds;
        if (last) last[o] = m->last[i];
        if (xyz) { xyz[3 * o] = c.sx; xyz[3 * o + 1] = c.sy; xyz[3 * o + 2] = c.sz; }
        if (cov) for (int k = 0; k < 6; ++k) cov[6 * o + k] = m->cov[i].v[k];
        if (rgb) for (int k = 0; k < 4; ++k) rgb[4 * o + k] = m->color[i].v[k];
        if (inten) inten[o] = m->intensity[i];
        ++o;
    }
    return o;
}

// the voxel key of every point after the transform (the invalid key for a skipped point)
void ogm_restate_point_keys(void* h, const float* pts, uint64_t n, const float* pose16, uint64_t* keys_out) {
    const Map* m = static_cast<Map*>(h);
    for (uint64_t i = 0; i < n; ++i) {
        float w[4];
        Map::world_point(pts + 4 * i, pose16, w);
        keys_out[i] = oracle::compute_voxel_bit(w, m->inv);
    }
}

// The bounded walk alone: the cells stepped into from origin3 towards target3, the target's cell last, three ints per cell, at most
// `cap` of them written. Returns the number of steps taken.
uint64_t ogm_restate_walk(const float* origin3, const float* target3, float inv_voxel, int32_t* cells_out, uint64_t cap) {
    uint64_t k = 0;
    return bounded_walk(origin3[0], origin3[1], origin3[2], target3[0], target3[1], target3[2], inv_voxel, [&](int x, int y, int z) {
        if (k < cap) { cells_out[3 * k] = x; cells_out[3 * k + 1] = y; cells_out[3 * k + 2] = z; }
        ++k;
    });
}

// The reference's own loop (:880-899) with a step budget, for the test that shows where it does not end: returns the steps taken, or
// `budget` when it had not landed on the target's cell by then.
uint64_t ogm_reference_walk_steps(const float* origin3, const float* target3, float inv_voxel, uint64_t budget) {
    const float sox = origin3[0] * inv_voxel, soy = origin3[1] * inv_voxel, soz = origin3[2] * inv_voxel;
    const float stx = target3[0] * inv_voxel, sty = target3[1] * inv_voxel, stz = target3[2] * inv_voxel;
    long long ix = (long long)std::floor(sox), iy = (long long)std::floor(soy), iz = (long long)std::floor(soz);
    const long long tx = (long long)std::floor(stx), ty = (long long)std::floor(sty), tz = (long long)std::floor(stz);
    if (ix == tx && iy == ty && iz == tz) return 0;
    const float dir_x = stx - sox, dir_y = sty - soy, dir_z = stz - soz;
    const float ax = std::fabs(dir_x), ay = std::fabs(dir_y), az = std::fabs(dir_z);
    const int step_x = (dir_x > 0.0f) ? 1 : ((dir_x < 0.0f) ? -1 : 0);
    const int step_y = (dir_y > 0.0f) ? 1 : ((dir_y < 0.0f) ? -1 : 0);
    const int step_z = (dir_z > 0.0f) ? 1 : ((dir_z < 0.0f) ? -1 : 0);
    const float frac_x = sox - std::floor(sox), frac_y = soy - std::floor(soy), frac_z = soz - std::floor(soz);
    const float inf = INFINITY;
    const float inv_x = (ax > FLT_EPSILON) ? (1.0f / ax) : inf, inv_y = (ay > FLT_EPSILON) ? (1.0f / ay) : inf,
                inv_z = (az > FLT_EPSILON) ? (1.0f / az) : inf;
    float t_max_x = (step_x != 0) ? ((step_x > 0 ? (1.0f - frac_x) : frac_x) * inv_x) : inf;
    float t_max_y = (step_y != 0) ? ((step_y > 0 ? (1.0f - frac_y) : frac_y) * inv_y) : inf;
    float t_max_z = (step_z != 0) ? ((step_z > 0 ? (1.0f - frac_z) : frac_z) * inv_z) : inf;
    const float t_delta_x = (step_x != 0) ? inv_x : inf, t_delta_y = (step_y != 0) ? inv_y : inf, t_delta_z = (step_z != 0) ? inv_z : inf;
    for (uint64_t s = 1; s <= budget; ++s) {
        if (t_max_x <= t_max_y && t_max_x <= t_max_z) { ix += step_x; t_max_x += t_delta_x; }
        else if (t_max_y <= t_max_z) { iy += step_y; t_max_y += t_delta_y; }
        else { iz += step_z; t_max_z += t_delta_z; }
        if (ix == tx && iy == ty && iz == tz) return s;
    }
    return budget;
}

}  // extern "C"
