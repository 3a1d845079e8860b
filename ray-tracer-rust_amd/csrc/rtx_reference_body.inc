// rtx_reference_body.inc — reference_tiles_kernel's body (rtx_kernel.hip), as text: included once by
// rtx::reference_tiles_kernel with `out` the frame's RGB8 bytes, and once by rtxo::reference_records_kernel with `out` a
// RecordOut (rtx_pass_helpers.hpp), whose hit count is this loop's own.  (Text and not a __device__ template:
// rtx_pass_shade.hpp says why.)
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    const bool have_ref = S.n_ref_nodes != 0u;
    const NodeRec RTX_CONSTANT *stream = (const NodeRec RTX_CONSTANT *)(have_ref ? S.ref_nodes : S.nodes);
    const uint32_t n_stream = have_ref ? S.n_ref_nodes : S.n_nodes;
    const uint32_t lane = threadIdx.x;
    const uint32_t n_redo = __builtin_amdgcn_readfirstlane(redo[kQueueRedoCount]);
    WaveCounters wc;
    unsigned long long primary_hits = 0;
    for (uint32_t q = blockIdx.x; q < n_redo; q += gridDim.x) {
        const uint32_t tid = __builtin_amdgcn_readfirstlane(redo[kQueueHeader + q]);
        uint32_t px, py, ly;
        uint32_t tile_x, tile_y;
        tile_xy(tid, tiles_x, tile_blocks, tile_x, tile_y);
        const bool in_frame = tile_pixel(S, ts, tile_x, tile_y, lane, px, py, ly);
        float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
        uint32_t n_hits = 0u;
        const float denom = (float)(S.nb_ray * S.nb_light);
        for (uint32_t r = 0; r < S.nb_ray; ++r) {
            float dx, dy, dz, t;
            uint32_t idx;
            primary_ray(S, in_frame, px, py, r, dx, dy, dz);
            closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, in_frame, S.eye[0], S.eye[1], S.eye[2],
                                         dx, dy, dz, t, idx, wc);
            const bool hit = in_frame && idx != kNone;
            const unsigned long long hit_mask = ballot(hit);
            if (hit_mask == 0ull) continue;
            if (COUNT) primary_hits += __popcll(hit_mask);
            if (std::is_same<decltype(out), const RecordOut>::value && hit) ++n_hits;
            float hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
            if (hit) {
                hx = S.eye[0] + t * dx;
                hy = S.eye[1] + t * dy;
                hz = S.eye[2] + t * dz;
                const ShadeRec sh = S.shade[idx];
                hit_normal<SPHERES>(sh, hx, hy, hz, nx, ny, nz);
                cr = sh.rgb[0]; cg = sh.rgb[1]; cb = sh.rgb[2];
            }
            for (uint32_t i = 0; i < S.nb_light; ++i) {
                const float *lp = S.light_points + 3u * (r * S.nb_light + i);
                const float vx = lp[0] - hx, vy = lp[1] - hy, vz = lp[2] - hz;
                const float dist_light = sqrtf(vx * vx + vy * vy + vz * vz);
                const float sx = vx / dist_light, sy = vy / dist_light, sz = vz / dist_light;
                float st;
                uint32_t sidx;
                closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, hit, hx, hy, hz, sx, sy, sz,
                                             st, sidx, wc);
                const float lnd = fabsf(nx * sx + ny * sy + nz * sz);
                bool lit = true;
                if (sidx != kNone) {
                    const float qx = hx - (hx + st * sx), qy = hy - (hy + st * sy), qz = hz - (hz + st * sz);
                    lit = sqrtf(qx * qx + qy * qy + qz * qz) > dist_light;
                }
                if (hit && lit) {
                    acc_r = acc_r + ((cr * lnd) / denom);
                    acc_g = acc_g + ((cg * lnd) / denom);
                    acc_b = acc_b + ((cb * lnd) / denom);
                }
            }
        }
        if (in_frame) store_pixel(S, S.gamma_thr, out, px, ly, acc_r, acc_g, acc_b, n_hits);
    }
    if (COUNT && lane == 0) flush_counters<COUNT>(counters, primary_hits, wc);
