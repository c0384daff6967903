// The linearisation of ONE source point against a VoxelHashMap's registration rows, as statements: included, not called. In scope
// where it is included: the template arguments LOSS, P2D, NV; VhmRegArgs A; Rigid T; unsigned i (the point); float acc[kAcc - 1];
// unsigned cnt; and the macro VHM_POINT_DONE, the statement that ends the point (`continue` in a point loop, `return` in a function).
// Transform, the NV cell keys, every cell's first probe, find_slot's remaining probes, the nearest counting mean, the distance
// gate, the winner's covariance rows, linearize_terms into acc. The winner's slot goes to A.slots[i].
// Why statements and not only a function: vhm_linearize_kernel (voxel_registration.hip) needs them in place. Through a function the
// compiler allocates 98-102 registers at 7 cells and 179-187 at 27, against 92-96 and 156-164 in place (the first-probe slots
// then stay one 27-register vector across the point loop), and 168 is what three waves a SIMD leave a lane
// (tests/test_voxel_registration_cpu.py). One text, two users: vhm_linearize_point (sp_voxel_registration.h) wraps it for the
// one-workgroup-per-hypothesis kernel. No include guard on purpose.
    const float4 p = A.src[i];
    float qx, qy, qz;
    transform_point(T, p.x, p.y, p.z, qx, qy, qz);
    unsigned best = kNoFrozenSlot;
    uint64_t best_key = kInvalidKey;
    float best_d2 = INFINITY, tx = 0.0f, ty = 0.0f, tz = 0.0f;
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        const int64_t c0 = (int64_t)floorf(qx * A.inv) + kCellOffset;
        const int64_t c1 = (int64_t)floorf(qy * A.inv) + kCellOffset;
        const int64_t c2 = (int64_t)floorf(qz * A.inv) + kCellOffset;
        // every cell's first probe: the loads leave together, nothing is compared before the last one has been issued
        unsigned s0[NV];
        uint64_t k0[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const uint64_t h = cell_key(c0 + kCellOffsets.d[j][0], c1 + kCellOffsets.d[j][1], c2 + kCellOffsets.d[j][2]);
            s0[j] = h == kInvalidKey ? kNoFrozenSlot : (unsigned)slot_id(h, 0, A.capacity);
            k0[j] = h == kInvalidKey ? kInvalidKey : A.keys[s0[j]];
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (s0[j] == kNoFrozenSlot) continue;  // a cell outside the key's range
            const uint64_t h = cell_key(c0 + kCellOffsets.d[j][0], c1 + kCellOffsets.d[j][1], c2 + kCellOffsets.d[j][2]);
            unsigned long long s = s0[j];
            if (k0[j] != h) {  // find_slot<100> from its second probe on
                s = kNoSlot;
                if (k0[j] != kInvalidKey)
                    for (unsigned pr = 1; pr < kVhmMaxProbe; ++pr) {
                        const unsigned long long sp = slot_id(h, pr, A.capacity);
                        const uint64_t k = A.keys[sp];
                        if (k == h) { s = sp; break; }
                        if (k == kInvalidKey) break;
                    }
            }
            if (s == kNoSlot) continue;
            const float4 m = A.rows[3 * (size_t)s];
            if (m.w != 1.0f) continue;
            const float d2 = dist2(qx, qy, qz, m.x, m.y, m.z);
            if (d2 < best_d2) {  // strict: an exact tie stays with the earlier cell
                best_d2 = d2; best = (unsigned)s; best_key = h;
                tx = m.x; ty = m.y; tz = m.z;
            }
        }
    }
    if (best != kNoFrozenSlot && best_d2 > A.max_d2) { best = kNoFrozenSlot; best_key = kInvalidKey; }
    A.slots[i] = best;
    if (A.corr_keys) A.corr_keys[i] = best_key;
    if (best == kNoFrozenSlot) VHM_POINT_DONE;
    const Sym3 Ct = load_sym(A.rows + 3 * (size_t)best + 1);
    Sym3 Cs{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (!P2D) Cs = load_sym(A.src_rows + 2 * (size_t)i);
    float t[kLinTerms];
    linearize_terms<LOSS, P2D, false, kLinTerms>(T, p.x, p.y, p.z, qx, qy, qz, tx, ty, tz, Cs, Ct, A.scale, t);
#pragma unroll
    for (int e = 0; e < kLinTerms; ++e) acc[e] += t[e];
    ++cnt;
