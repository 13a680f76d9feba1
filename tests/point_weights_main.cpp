// Runs the weight entries' value check (csrc/point_weights.h: scan_weights) on weights given by their bit patterns -- plain
// C++17, no HIP -- and prints what it found.  Built and run by tests/test_point_weights_cpu.py.
//   point_weights f32|f64 [hex bits of weight 0] [hex bits of weight 1] ...
// One line: verdict=<OK|BAD_VALUE|ALL_ZERO|SUM_NOT_FINITE> index=<i> value=<hex bits of a double> sum=<hex bits of a double>
#include "point_weights.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T, class BITS>
static hgmm::WeightScan scan(int n, char** hex) {
    static_assert(sizeof(T) == sizeof(BITS), "bit pattern");
    std::vector<T> w((size_t)n);
    for (int i = 0; i < n; ++i) {
        const BITS b = (BITS)std::strtoull(hex[i], nullptr, 16);
        std::memcpy(&w[i], &b, sizeof b);
    }
    return hgmm::scan_weights(w.data(), (int64_t)n);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    hgmm::WeightScan s;
    if (!std::strcmp(argv[1], "f32")) s = scan<float, unsigned>(argc - 2, argv + 2);
    else if (!std::strcmp(argv[1], "f64")) s = scan<double, unsigned long long>(argc - 2, argv + 2);
    else return 2;
    static const char* const names[] = {"OK", "BAD_VALUE", "ALL_ZERO", "SUM_NOT_FINITE"};
    static_assert(hgmm::WEIGHTS_OK == 0 && hgmm::WEIGHTS_BAD_VALUE == 1 && hgmm::WEIGHTS_ALL_ZERO == 2 &&
                  hgmm::WEIGHTS_SUM_NOT_FINITE == 3, "names");
    unsigned long long value, sum;
    std::memcpy(&value, &s.value, sizeof value);
    std::memcpy(&sum, &s.sum, sizeof sum);
    std::printf("verdict=%s index=%lld value=%016llx sum=%016llx\n", names[s.verdict], (long long)s.index, value, sum);
    return 0;
}
