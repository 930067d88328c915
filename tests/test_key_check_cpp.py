"""check_key of include/groth16_snark_hip.hpp from a plain C++ program (host route, no device): a key made of the two generators
passes; a G1 point in b_g2_query is named with its index and code."""
import os
import subprocess
import textwrap

import numpy as np

from oracle import pyref as R
from tests.helpers import aff_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_key_in_a_cpp_program(tmp_path):
    (tmp_path / "in.bin").write_bytes(np.concatenate([aff_limbs(R.G1_GEN), aff_limbs(R.G2_GEN)]).astype(np.uint64).tobytes())
    src = tmp_path / "k.cpp"
    src.write_text(textwrap.dedent(r'''
        #include <cstdio>
        #include "groth16_snark_hip.hpp"
        int main(int argc, char** argv) {
          uint64_t in[48];
          FILE* f = std::fopen(argv[1], "rb");
          if (!f || std::fread(in, 8, 48, f) != 48) return 2;
          std::fclose(f);
          const uint64_t *g1 = in, *g2 = in + 24;
          std::vector<uint64_t> v1(48), v2(48);             // two variables: (g1, g1) and (g2, g2)
          for (int i = 0; i < 2; i++) { std::memcpy(&v1[i * 24], g1, 192); std::memcpy(&v2[i * 24], g2, 192); }
          zkhip_crs_desc pk{};
          pk.n_vars = 2; pk.n_primary = 0; pk.domain_size = 2;
          pk.alpha_g1 = pk.beta_g1 = pk.delta_g1 = g1; pk.beta_g2 = pk.delta_g2 = g2;
          pk.a_query = pk.b_g1_query = pk.h_query = pk.l_query = v1.data(); pk.b_g2_query = v2.data();
          zkhip_key_report rep = zecale_amd::check_key(pk, nullptr, nullptr, true);
          std::printf("good: ok=%d %s\n", rep.ok, zecale_amd::key_report_message(rep).c_str());
          std::memcpy(&v2[24], g1, 192);                    // a G1 point in the B-G2 vector
          rep = zecale_amd::check_key(pk, nullptr, nullptr, true);
          std::printf("bad: ok=%d %s\n", rep.ok, zecale_amd::key_report_message(rep).c_str());
          try { zkhip_crs_desc none{}; zecale_amd::check_key(none, nullptr, nullptr, true); } catch (const std::runtime_error& e) { std::printf("%s\n", e.what()); }
          return 0;
        }
    '''))
    exe = tmp_path / "k"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "zecale_amd"), "-lzkhip", "-Wl,-rpath," + os.path.join(ROOT, "zecale_amd")])
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "good: ok=1 key check: ok"
    assert lines[1].startswith("bad: ok=0") and "b_g2_query[1]: OFF_CURVE" in lines[1] and "b_g1_query/b_g2_query: not evaluated" in lines[1]
    assert "zkhip_crs_check_host: bad argument" in lines[2]
