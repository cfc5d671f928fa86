// One pass of scm_kernel (mvdr.hip) over the group's frame list, included there once per pass with `LO`, the first packed entry
// of the pass, a constant in scope: the walk over the list with the accumulators of the entries [LO, LO + E), the reduce-scatter
// over the 16 lanes and the totals' way into LDS.  (Text inclusion and not a function or a loop over the passes: either one
// changed the NC = 7 kernels' schedule; included once with LO = 0 they are, instruction for instruction, what they were.)
    double acc[E], pl[E];
#pragma unroll
    for (int i = 0; i < E; ++i) { acc[i] = 0.0; pl[i] = 0.0; }
    const int nk = k == 0 ? cnt[0] : (k == 1 ? cnt[1] : (k == 2 ? cnt[2] : cnt[3]));
    const bool upper = l16 >= 8;
    for (int i = l16; i < nk; i += 16) {
        const unsigned e = lists[k * TS + i];
        const int t = e & 0x7fff;
        const double first_ = (e & 0x8000) ? 1.0 : 0.0;
        const double w_ = (double)ms[k * TS + t] - 1e-10;
        const double w = upper ? first_ : w_, first = upper ? w_ : first_;   // (names as in the lower half)
        double xr[NC], xi[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { xr[c] = (double)xs[c * TS + t]; xi[c] = (double)xs[(NC + c) * TS + t]; }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c >= LO && c < LO + E) {
                const double p = xr[c] * xr[c] + xi[c] * xi[c];
                acc[c - LO] += w * p;
                pl[c - LO] += first * p;
            }
        }
        int p = NC;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int d = c + 1; d < NC; ++d) {
                if (p >= LO && p < LO + E) {      // (NC and E are even or the pass is the only one: a pair never straddles passes)
                    const double pr = xr[c] * xr[d] + xi[c] * xi[d];      // Re x_c conj(x_d)
                    const double pi = xi[c] * xr[d] - xr[c] * xi[d];      // Im
                    acc[p - LO] += w * pr; pl[p - LO] += first * pr;
                    acc[p + 1 - LO] += w * pi; pl[p + 1 - LO] += first * pi;
                }
                p += 2;
            }
        }
    }
    // ---- reduce-scatter over the group's 16 lanes: four DPP exchanges, each halving the number of values a lane keeps
    // (summing all 98 values into all 16 lanes cost 4 x 98 exchanges and 16 copies of every total; this costs
    // 49 + 25 + 13 + 7 and leaves each total in one lane).  A lane keeps the lower or upper half of its values by one bit
    // of its position; its partner keeps the other half and sends the half this lane keeps.
    // value list: acc[0..E-1] then pl[0..E-1]; after the steps lane l holds the totals of original indices
    //   j + E b0 + H1 b1 + H2 b2 + H3 b3,  j = 0..H3-1,  b0 = l16 >= 8, b1 = (l16 & 7) >= 4, b2 = bit 1, b3 = bit 0
    // (E, H1, H2, H3 = 49, 25, 13, 7 at NC = 7)
    double v1[E], v2[H1], v3[H2], v4[H3];
    {
        // partner: 15 - l16 (row_mirror), in the other half: its `pl` is what this lane's `acc` is (see above)
#pragma unroll
        for (int j = 0; j < E; ++j) v1[j] = acc[j] + dpp_get<0x140>(pl[j]);
    }
    {
        const bool up = (l16 & 7) >= 4;      // partner: 7 - (l16 & 7) inside the half row (row_half_mirror)
#pragma unroll
        for (int j = 0; j < H1; ++j) {
            const double lo = v1[j], hi = j + H1 < E ? v1[j + H1] : 0.0;
            const double keep = up ? hi : lo, send = up ? lo : hi;
            v2[j] = keep + dpp_get<0x141>(send);
        }
    }
    {
        const bool up = (l16 & 2) != 0;      // partner: l16 ^ 2 (quad_perm [2,3,0,1])
#pragma unroll
        for (int j = 0; j < H2; ++j) {
            const double lo = v2[j], hi = j + H2 < H1 ? v2[j + H2] : 0.0;
            const double keep = up ? hi : lo, send = up ? lo : hi;
            v3[j] = keep + dpp_get<0x4E>(send);
        }
    }
    {
        const bool up = (l16 & 1) != 0;      // partner: l16 ^ 1 (quad_perm [1,0,3,2])
#pragma unroll
        for (int j = 0; j < H3; ++j) {
            const double lo = v3[j], hi = j + H3 < H2 ? v3[j + H3] : 0.0;
            const double keep = up ? hi : lo, send = up ? lo : hi;
            v4[j] = keep + dpp_get<0xB1>(send);
        }
    }
    // the totals meet in LDS: tot[k][0 .. NPACK) weighted sums, tot[k][NPACK .. 2 NPACK) plain sums
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    {
        const int base = (l16 >= 8 ? NPACK : 0) + LO;
        const int o1 = ((l16 & 7) >= 4 ? H1 : 0), o2 = ((l16 & 2) ? H2 : 0), o3 = ((l16 & 1) ? H3 : 0);
#pragma unroll
        for (int j = 0; j < H3; ++j) {
            // position inside the pass's E values after steps 2..4; slots past a half's end were padding (zero sums)
            const int q3 = j + o3, q2 = q3 + o2, q1 = q2 + o1;
            const bool real = q3 < H2 && q2 < H1 && q1 < E && LO + q1 < NPACK;
            if (real) tot[k * (2 * NPACK) + base + q1] = v4[j];
        }
    }
