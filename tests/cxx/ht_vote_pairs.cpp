// The vote pairs of LinePencilModel::get_weights (reference line_pencil.cpp:53-59) from the C++ library itself:
// std::mt19937, default seeded, through std::uniform_int_distribution<int>(0, n - 1).  tests/numpy_estimators_ref.py
// restates both in Python integers; test_estimators_second_source_cpu.py compiles this and compares.
// Output: the 10000th output of a default-seeded engine (the standard's known answer, 4123659995), then for every n
// on the command line a line "n <n>" and <pairs> lines "a b".
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char** argv) {
    std::mt19937 check;
    check.discard(9999);
    std::printf("%lu\n", (unsigned long)check());
    const int pairs = argc > 1 ? std::atoi(argv[1]) : 0;
    for (int k = 2; k < argc; ++k) {
        const int n = std::atoi(argv[k]);
        std::mt19937 rng;
        std::uniform_int_distribution<int> rand_idx(0, n - 1);
        std::printf("n %d\n", n);
        for (int i = 0; i < pairs; ++i) {
            const int a = rand_idx(rng);
            const int b = rand_idx(rng);
            std::printf("%d %d\n", a, b);
        }
    }
    return 0;
}
