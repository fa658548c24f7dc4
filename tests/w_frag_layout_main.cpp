// Stand-alone CPU check of the fragment-ordered weight image layouts
// (csrc/w_frag.h): for each N:K argument the entry -> (row, col) maps of the
// forward and the dz image must be bijections onto the padded matrix, and the
// index functions the k-loops use must agree with the coordinate functions the
// writers use. Prints one "N K fwd_entries dz_entries ok" line per argument;
// exit status 1 on the first violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "w_frag.h"

using namespace rt::wfrag;

static int fail(const char* what, int n, int k, long long e) {
    std::fprintf(stderr, "%s at n=%d k=%d entry=%lld\n", what, n, k, e);
    return 1;
}

static int check(int n, int k) {
    {   // forward image of W[n][k]: rows padded to 32·T, columns to 32·S, 4 columns per entry
        const int R = 32 * fwd_tiles(n), C = 32 * fwd_steps(k);
        const long long tot = fwd_entries(n, k);
        if (tot * 4 != static_cast<long long>(R) * C) return fail("fwd size", n, k, tot);
        std::vector<char> seen(static_cast<size_t>(R) * C, 0);
        for (long long e = 0; e < tot; ++e) {
            int row, col;
            fwd_coords(k, e, row, col);
            if (row < 0 || row >= R || col < 0 || col + 3 >= C || (col % 4) != 0) return fail("fwd range", n, k, e);
            for (int q = 0; q < 4; ++q) {
                char& s = seen[static_cast<size_t>(row) * C + col + q];
                if (s) return fail("fwd duplicate", n, k, e);
                s = 1;
            }
            // the address the k-loop forms: tile t, iteration s, load j, lane l
            const int l = static_cast<int>(e & 63), j = static_cast<int>((e >> 6) & 3);
            const int t = row / 32, s = col / 32;
            if (fwd_index(k, t, s, j, l) != e) return fail("fwd index", n, k, e);
            const int c = l & 31, h = l >> 5;
            if (row != 32 * t + c || col != 32 * s + 16 * (j >> 1) + 8 * h + 4 * (j & 1)) return fail("fwd lane", n, k, e);
        }
        for (char s : seen)
            if (!s) return fail("fwd hole", n, k, -1);
    }
    {   // dz image of Wᵀ[k][n]: rows padded to 32·KT, columns to 16·NS
        const int R = 32 * dz_tiles(k), C = 16 * dz_steps(n);
        const long long tot = dz_entries(n, k);
        if (tot * 4 != static_cast<long long>(R) * C) return fail("dz size", n, k, tot);
        std::vector<char> seen(static_cast<size_t>(R) * C, 0);
        for (long long e = 0; e < tot; ++e) {
            int trow, tcol;
            dz_coords(n, e, trow, tcol);
            if (trow < 0 || trow >= R || tcol < 0 || tcol + 3 >= C || (tcol % 4) != 0) return fail("dz range", n, k, e);
            for (int q = 0; q < 4; ++q) {
                char& s = seen[static_cast<size_t>(trow) * C + tcol + q];
                if (s) return fail("dz duplicate", n, k, e);
                s = 1;
            }
            const int l = static_cast<int>(e & 63), j = static_cast<int>((e >> 6) & 1);
            const int kt = trow / 32, sb = tcol / 16;
            if (dz_index(n, kt, sb, j, l) != e) return fail("dz index", n, k, e);
            const int c = l & 31, h = l >> 5;
            if (trow != 32 * kt + c || tcol != 16 * sb + 8 * h + 4 * j) return fail("dz lane", n, k, e);
        }
        for (char s : seen)
            if (!s) return fail("dz hole", n, k, -1);
    }
    std::printf("%d %d %lld %lld ok\n", n, k, static_cast<long long>(fwd_entries(n, k)),
                static_cast<long long>(dz_entries(n, k)));
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        int n = 0, k = 0;
        if (std::sscanf(argv[i], "%d:%d", &n, &k) != 2 || n <= 0 || k <= 0) {
            std::fprintf(stderr, "bad argument %s (want N:K)\n", argv[i]);
            return 2;
        }
        if (check(n, k)) return 1;
    }
    return 0;
}
