"""zkhip_key_opts grew a fifth field, table_model, behind the four it had: the C struct, ZKHIP_KEY_OPTS_DEFAULT, the ctypes mirror and
the server's --key-table-model flag must agree on its place and its default (0: XYZZ, today's behaviour).  CPU only."""
import ctypes
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["precompute", "table_naf", "window", "batch_msms", "table_model"]


def test_c_struct_size_default_and_field_order(tmp_path):
    src = tmp_path / "opts.cpp"
    src.write_text(textwrap.dedent(r'''
        #include <cstddef>
        #include <cstdio>
        #include "zkhip.h"
        static_assert(sizeof(zkhip_key_opts) == 5 * sizeof(int), "five ints, no padding");
        int main() {
          zkhip_key_opts d = ZKHIP_KEY_OPTS_DEFAULT;
          zkhip_key_opts four = {1, 0, 13, 0};              // an initialiser written for the four earlier fields
          zkhip_key_opts zero = {};
          if (d.precompute != -1 || d.table_naf != -1 || d.window != 0 || d.batch_msms != -1 || d.table_model != 0) return 1;
          if (four.precompute != 1 || four.table_naf != 0 || four.window != 13 || four.batch_msms != 0 || four.table_model != 0) return 2;
          if (zero.table_model != 0) return 3;
          std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(zkhip_key_opts), offsetof(zkhip_key_opts, precompute), offsetof(zkhip_key_opts, table_naf),
                      offsetof(zkhip_key_opts, window), offsetof(zkhip_key_opts, batch_msms), offsetof(zkhip_key_opts, table_model));
          return 0;
        }
    '''))
    exe = tmp_path / "opts"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    size, *offsets = (int(x) for x in out.stdout.split())
    from zecale_amd import zkhip
    assert [f for f, _ in zkhip.KeyOpts._fields_] == FIELDS
    assert all(t is ctypes.c_int for _, t in zkhip.KeyOpts._fields_)
    assert ctypes.sizeof(zkhip.KeyOpts) == size == 5 * ctypes.sizeof(ctypes.c_int)
    assert [getattr(zkhip.KeyOpts, f).offset for f in FIELDS] == offsets


def test_python_key_opts():
    from zecale_amd import zkhip
    as_list = lambda o: [getattr(o, f) for f in FIELDS]
    assert as_list(zkhip.key_opts()) == [-1, -1, 0, -1, 0]
    assert as_list(zkhip.KeyOpts(-1, -1, 0, -1)) == [-1, -1, 0, -1, 0]            # four positional values: the fifth stays 0
    assert as_list(zkhip.key_opts(precompute=True, table_naf=False, window=13, batch_msms=False)) == [1, 0, 13, 0, 0]
    assert zkhip.key_opts(table_model=1).table_model == 1 and zkhip.key_opts(table_model="edwards").table_model == 1
    assert zkhip.key_opts(table_model=0).table_model == 0 and zkhip.key_opts(table_model="xyzz").table_model == 0
    with pytest.raises(KeyError):
        zkhip.key_opts(table_model="jacobian")


def test_server_flag_parses_to_the_key_options(monkeypatch):
    from zecale_amd import server
    as_list = lambda o: [getattr(o, f) for f in FIELDS]
    parse = lambda argv: server.main(argv, parse_only=True)
    monkeypatch.delenv("ZKHIP_TABLE_NAF", raising=False)
    dflt = parse([])
    assert dflt.key_table_model == "xyzz"
    assert as_list(server.server_key_opts(dflt.key_table_model)) == [-1, 1, 0, -1, 0]         # as before the flag: every-bit-position tables
    assert as_list(server.server_key_opts()) == [-1, 1, 0, -1, 0]
    edw = parse(["--key-table-model", "edwards"])
    assert edw.key_table_model == "edwards"
    assert as_list(server.server_key_opts(edw.key_table_model)) == [-1, 0, 0, -1, 1]          # one level per window, Edwards forms
    assert parse(["--key-table-model", "xyzz"]).key_table_model == "xyzz"
    with pytest.raises(SystemExit):
        parse(["--key-table-model", "jacobian"])
    monkeypatch.setenv("ZKHIP_TABLE_NAF", "0")                                                  # the environment decides the XYZZ key's kind ...
    assert as_list(server.server_key_opts("xyzz")) == [-1, -1, 0, -1, 0]
    assert as_list(server.server_key_opts("edwards")) == [-1, 0, 0, -1, 1]                    # ... never the Edwards key's
    with pytest.raises(ValueError):
        server.server_key_opts("jacobian")
