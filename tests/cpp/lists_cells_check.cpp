// lists_cells_check.cpp -- host/lists_cells_rule.h as a program of its own (tests/test_lists_cells_rule.py builds it under
// ASan + UBSan): one line per query on the command line, "nb S F mean_units" -> "choice lambda p".
#include "../../bucket-map_amd/host/lists_cells_rule.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: lists_cells_check nb S F mean_units [nb S F mean_units ...]\n");
        return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
        const uint32_t nb = (uint32_t)strtoul(argv[i], nullptr, 10), S = (uint32_t)strtoul(argv[i + 1], nullptr, 10),
                       F = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
        const double mean_units = strtod(argv[i + 3], nullptr);
        double lambda = 0.0, p = 0.0;
        const int choice = bmf_rule::lists_cells(nb, S, F, mean_units, &lambda, &p);
        printf("%d %.17g %.17g\n", choice, lambda, p);
    }
    return 0;
}
