// Compiles ria_amd/csrc/cfo_theta0.h for the host.  Reads lines "<cfo_hz bit pattern, hex> <abs_position, decimal>" from
// stdin and prints the bit pattern of cfo_theta0() for each (tests/test_cfo_theta0_host.py compares them with the oracle).
#include "../../ria_amd/csrc/cfo_theta0.h"
#include <cinttypes>
#include <cstdio>
int main() {
    uint32_t cfo_bits;
    uint64_t pos;
    while (scanf("%" SCNx32 " %" SCNu64, &cfo_bits, &pos) == 2)
        printf("%08" PRIx32 "\n", ria::f2u(ria::cfo_theta0(ria::u2f(cfo_bits), pos)));
    return 0;
}
