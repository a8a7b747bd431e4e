// nmpc_dwa_step.inl -- the body of the dynamic-window step, included by nmpc_dwa.h into each of its two kernels with
// `p` (DwaParams<T> or DwaListsParams<T>) and the compile-time constant LISTS in scope. LISTS = false: modes 0 .. 2, the
// rectangular rows read from global memory. LISTS = true: the per-offset lists staged in LDS (nmpc_dwa.h, "Per-offset lists").
// It is text and not a function on purpose: called through a function, even a force-inlined one, the kernels for modes 0 .. 2
// come out of the compiler with other registers and another instruction order than before; included, they keep their bytes.
    extern __shared__ __align__(16) unsigned char dwa_smem[];
    T* edges = reinterpret_cast<T*>(dwa_smem);
    const int n_edge = 4 * p.M;
    for (int e = threadIdx.x; e < n_edge; e += kDwaThreads) {
        const T* q = p.polys + (size_t)(e >> 2) * 8;
        const int k = e & 3, k1 = (k + 1) & 3;
        const T ax = q[2 * k], ay = q[2 * k + 1], bx = q[2 * k1], by = q[2 * k1 + 1];
        const T len = thypot(bx - ax, by - ay);
        T* o = edges + (size_t)e * kDwaEdgeReals;
        o[0] = ax, o[1] = ay, o[2] = bx, o[3] = by, o[4] = (bx - ax) / len, o[5] = (by - ay) / len;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * (kDwaThreads / 64) + (threadIdx.x >> 6);
    if (a >= p.n_run) return;
    const long long bl = p.run ? p.run[a] : a;
    if (bl < 0 || bl >= p.B) return; // (a device-side run list is not validated by the host: stay inside the arrays)
    const size_t b = (size_t)bl;
    const int N = p.N, H = p.H;
    const T inf = T(INFINITY);
    const T x0 = p.state_c[3 * (size_t)a], y0 = p.state_c[3 * (size_t)a + 1], th0 = p.state_c[3 * (size_t)a + 2];
    const T gx = p.goal[2 * b], gy = p.goal[2 * b + 1];
    // base speed: 0.8 lin_vel_max, lowered near the goal (trajectory_tracker.py:312-316)
    T base = p.base_speed;
    {
        const T dg = thypot(x0 - gx, y0 - gy);
        if (dg < base * T(N) * p.tsT) {
            const T sp = T(2) * dg / T(N) / p.tsT;
            base = sp < p.lin_vel_max ? sp : p.lin_vel_max;
        }
    }
    // window and grid in double
    double v0, v1, w0, w1, dvd, dwd;
    int nv, nw;
    dwa_window((double)p.last_u_c[2 * (size_t)a], p.acc, p.ts, p.vmin, p.vmax, v0, v1);
    dwa_window((double)p.last_u_c[2 * (size_t)a + 1], p.wacc, p.ts, -p.wmax, p.wmax, w0, w1);
    dwa_arange(v0, v1, p.dv, p.cap, nv, dvd);
    dwa_arange(w0, w1, p.dw, p.cap, nw, dwd);
    if (nv > 0 && nw > p.cap / nv) nw = p.cap / nv; // (never with the host's bound on cap: keeps the writes inside [cap])
    const int n_cand = nv * nw;
    long long plen = p.path_len[b];
    plen = plen < 2 ? 2 : plen > p.Pmax ? p.Pmax : plen;
    const T* path = p.path + b * (size_t)p.Pmax * 2;
    const T* dyn = p.dyn_c + (size_t)a * H * (size_t)(N + 1) * 6;
    const size_t hstride = (size_t)(N + 1) * 6;
    // LISTS: this wavefront's part of LDS behind the edge table -- the means, compacted [offset][row][2], and behind the
    // means of all four wavefronts the clamped counts [N + 1] and their running sums [N + 1]. The part is private to the
    // wavefront, whose LDS operations execute in program order: wave_barrier() only keeps the compiler from moving them.
    const T* means = nullptr;
    const int *lcnt = nullptr, *lstart = nullptr;
    int n_cur = 0;
    if constexpr (LISTS) {
        const int NP1 = N + 1, R = p.R, wave = threadIdx.x >> 6;
        T* lists = edges + (size_t)n_edge * kDwaEdgeReals;
        T* mw = lists + (size_t)wave * 2 * R * NP1;
        int* cw = reinterpret_cast<int*>(lists + (size_t)(kDwaThreads / 64) * 2 * R * NP1) + wave * 2 * NP1;
        int* sw = cw + NP1;
        const int* dc = p.dyn_count + (size_t)a * NP1;
        for (int t = lane; t < NP1; t += 64) {
            const int c = dc[t];
            cw[t] = c < 0 ? 0 : c > R ? R : c; // (device memory, not validated by the host: stay inside the rows)
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < NP1; t += 64) {
            int s = 0;
            for (int u = 0; u < t; ++u) s += cw[u];
            sw[t] = s;
        }
        __builtin_amdgcn_wave_barrier();
        const T* rows = p.dyn_c + (size_t)a * R * (size_t)NP1 * 6;
        for (int i = lane; i < R * NP1; i += 64) { // (neighbouring lanes take neighbouring offsets of one row)
            const int r = i / NP1, t = i - r * NP1;
            if (r < cw[t]) {
                const T* src = rows + (size_t)i * 6;
                T* dst = mw + 2 * (size_t)(sw[t] + r);
                dst[0] = src[0], dst[1] = src[1];
            }
        }
        __builtin_amdgcn_wave_barrier();
        means = mw, lcnt = cw, lstart = sw;
        n_cur = __builtin_amdgcn_readfirstlane(cw[0]);
    }

    T best = inf;
    int bidx = 0x7fffffff;
    for (int cnd = lane; cnd < n_cand; cnd += 64) {
        const int iv = cnd / nw, iw = cnd - iv * nw;
        const T v = (T)dwa_grid(v0, dvd, iv), w = (T)dwa_grid(w0, dwd, iw);
        T x = x0, y = y0, th = th0;
        T q_near = inf, h_near = inf, c_near = inf; // closest edge over all points: h^2 + c^2 and its components
        T q_cur = inf;                           // squared distance to the closest current position
        T d_steps = inf;                         // min_i sqrt(i + 1) * min_h |p_i - mu[h][i + 1]|
        const T kth = p.tsT * w;
        for (int i = 0; i <= N; ++i) {
            for (int e = 0; e < n_edge; ++e) {
                T h, c;
                dwa_edge(edges + (size_t)e * kDwaEdgeReals, x, y, h, c);
                const T q = h * h + c * c;
                if (q < q_near) q_near = q, h_near = h, c_near = c;
            }
            if constexpr (LISTS) {
                for (int hh = 0; hh < n_cur; ++hh) { // offset 0: the term of mode 1 over the count[0] current positions
                    const T ex = x - means[2 * hh], ey = y - means[2 * hh + 1];
                    const T q = ex * ex + ey * ey;
                    q_cur = q < q_cur ? q : q_cur;
                }
                if (i < N) { // offset i + 1: its count[i + 1] means lie side by side, broadcast reads
                    const int n = __builtin_amdgcn_readfirstlane(lcnt[i + 1]);
                    const T* m = means + 2 * (size_t)__builtin_amdgcn_readfirstlane(lstart[i + 1]);
                    T qs = inf;
                    for (int k = 0; k < n; ++k) {
                        const T fx = x - m[2 * k], fy = y - m[2 * k + 1];
                        const T q2 = fx * fx + fy * fy;
                        qs = q2 < qs ? q2 : qs;
                    }
                    const T di = tsqrt(qs) * tsqrt(T(i + 1)); // (an empty offset: inf, no d_i)
                    d_steps = di < d_steps ? di : d_steps;
                }
            } else if (p.dyn_mode >= 1) {
                T qs = inf;
                for (int hh = 0; hh < H; ++hh) {
                    const T* r = dyn + hh * hstride;
                    const T ex = x - r[0], ey = y - r[1];
                    const T q = ex * ex + ey * ey;
                    q_cur = q < q_cur ? q : q_cur;
                    if (p.dyn_mode == 2 && i < N) {
                        const T fx = x - r[6 * (i + 1)], fy = y - r[6 * (i + 1) + 1];
                        const T q2 = fx * fx + fy * fy;
                        qs = q2 < qs ? q2 : qs;
                    }
                }
                if (p.dyn_mode == 2 && i < N) {
                    const T di = tsqrt(qs) * tsqrt(T(i + 1));
                    d_steps = di < d_steps ? di : d_steps;
                }
            }
            if (i < N) { // unicycle RK4 with a constant control, stage by stage (motion_model.py:141-163)
                T s0, c0, s1, c1, s2, c2;
                tsincos(th, s0, c0);
                tsincos(th + T(0.5) * kth, s1, c1);
                tsincos(th + kth, s2, c2);
                const T k1x = p.tsT * (v * c0), k2x = p.tsT * (v * c1), k4x = p.tsT * (v * c2);
                const T k1y = p.tsT * (v * s0), k2y = p.tsT * (v * s1), k4y = p.tsT * (v * s2);
                x = x + T(1.0 / 6.0) * (k1x + T(2) * k2x + T(2) * k2x + k4x);
                y = y + T(1.0 / 6.0) * (k1y + T(2) * k2y + T(2) * k2y + k4y);
                th = th + T(1.0 / 6.0) * (kth + T(2) * kth + T(2) * kth + kth);
            }
        }
        // cost (trajectory_tracker.py:186-203): speed + goal direction + path deviation + static + dynamic
        const T c_speed = tabs(v - base) * p.q_speed;
        const T ang = tatan2(gy - y, gx - x) - th;
        T sa, ca;
        tsincos(ang, sa, ca);
        const T c_goal = tabs(tatan2(sa, ca)) * p.q_goal;
        T d_ref = inf;
        for (int j = 0; j + 1 < (int)plen; ++j) {
            const T ax = path[2 * j], ay = path[2 * j + 1], bx = path[2 * j + 2], by = path[2 * j + 3];
            const T len = thypot(bx - ax, by - ay);
            const T e[6] = {ax, ay, bx, by, (bx - ax) / len, (by - ay) / len};
            T h, c;
            dwa_edge(e, x, y, h, c);
            const T d = thypot(h, c);
            d_ref = d < d_ref ? d : d_ref; // (a NaN of a zero-length segment is skipped here; np.min would return it)
        }
        const T c_ref = d_ref * p.q_ref;
        T c_stc = T(0);
        if (n_edge > 0) {
            const T d = thypot(h_near, c_near);
            c_stc = d < T(0.05) ? inf : d > T(0.5) ? T(0) : T(1) / d * p.q_stc;
        }
        T c_dyn = T(0);
        if (LISTS || p.dyn_mode >= 1) {
            const T d = tsqrt(q_cur);
            const T c_cur = d > T(0.5) ? T(0) : d < T(0.2) ? inf : T(1) / d * p.q_dyn;
            T c_st = T(0);
            if (LISTS || p.dyn_mode == 2) c_st = d_steps < T(0.2) ? inf : d_steps > T(0.5) ? T(0) : T(1) / d_steps * p.q_dyn;
            c_dyn = c_st + c_cur;
        }
        const T cost = c_speed + c_goal + c_ref + c_stc + c_dyn;
        if (p.cost_all) p.cost_all[(size_t)a * p.cap + cnd] = cost;
        if (p.cand_all) {
            p.cand_all[((size_t)a * p.cap + cnd) * 2] = v;
            p.cand_all[((size_t)a * p.cap + cnd) * 2 + 1] = w;
        }
        if (cost < best) best = cost, bidx = cnd; // (a lane's candidates come in ascending order: strict keeps the first)
    }
    for (int s = 32; s > 0; s >>= 1) { // (cost, index) minimum, lowest index among equals
        const T ob = __shfl_xor(best, s, 64);
        const int oj = __shfl_xor(bidx, s, 64);
        if (ob < best || (ob == best && oj < bidx)) best = ob, bidx = oj;
    }
    T uv = T(0), uw = T(0);
    if (bidx != 0x7fffffff) {
        const int iv = bidx / nw, iw = bidx - iv * nw;
        uv = (T)dwa_grid(v0, dvd, iv), uw = (T)dwa_grid(w0, dwd, iw);
        if (tabs(uv) < p.stuck) uw = (T)(-p.wmax);
    }
    for (int e = lane; e < 2 * N; e += 64) p.U_c[(size_t)a * 2 * N + e] = (e & 1) ? uw : uv;
    if (lane == 0) {
        p.min_cost[a] = best;
        p.choice[a] = bidx == 0x7fffffff ? -1 : bidx;
        p.counts[2 * (size_t)a] = nv, p.counts[2 * (size_t)a + 1] = nw;
    }
