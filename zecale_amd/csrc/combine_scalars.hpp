// The scalars of a combined (random-combination) batch check, for both verifiers: pairing_host.hpp (BW6-761) and
// nested_combine_host.hpp (BLS12-377).  Host code only.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/random.h>

namespace zkhip {
namespace host {

// count x 16 bytes from the OS, each scalar redrawn while zero.  false: getrandom failed - there is no weaker generator behind it.
inline bool draw_rho(uint64_t* rho, size_t count) {
  for (size_t i = 0; i < count; i++) {
    do {
      size_t got = 0;
      while (got < 16) {
        const ssize_t n = getrandom(reinterpret_cast<char*>(rho + i * 2) + got, 16 - got, 0);
        if (n < 0 && errno == EINTR) continue;
        if (n <= 0) return false;
        got += (size_t)n;
      }
    } while ((rho[i * 2] | rho[i * 2 + 1]) == 0);
  }
  return true;
}

}  // namespace host
}  // namespace zkhip
