// spec_draft.h -- the prompt-lookup drafter of flm_generate_lookup (include/flm_gpu.h) in plain C++, written as the rule reads: the expected value of the device's
// k_spec_draft (csrc/flm_spec.h), exported through test_shim.cpp as fh_spec_draft.
#pragma once
#include <stdint.h>

namespace flmhost {

// h[0 .. n), n >= 1 -> d[0 .. k).  For g = min(ngram_max, n - 1) down to 1: the largest j with j + g <= n - 1 and h[j .. j + g) == h[n - g .. n); the first g with a
// match wins, with period p = n - g - j: d[i] = h[n - p + i] for i < p, else d[i - p].  No match at any g: d[i] = h[n - 1].
inline void spec_draft(const int32_t* h, int n, int k, int ngram_max, int32_t* d) {
    for (int g = ngram_max < n - 1 ? ngram_max : n - 1; g >= 1; --g)
        for (int j = n - 1 - g; j >= 0; --j) {
            bool same = true;
            for (int t = 0; t < g && same; ++t) same = h[j + t] == h[n - g + t];
            if (!same) continue;
            const int p = n - g - j;
            for (int i = 0; i < k; ++i) d[i] = i < p ? h[n - p + i] : d[i - p];
            return;
        }
    for (int i = 0; i < k; ++i) d[i] = h[n - 1];
}

} // namespace flmhost
