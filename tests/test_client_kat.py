"""Frozen outputs of the host-only client code and the key-file format, CPU only.

tests/golden/client_kat.json (tools/gen_client_kat.py) holds digests of everything one seeded client derives on the host:
keys of every kind, the first string in the three ciphertext formats with their host expansions, the host packing.  They
were recorded before the exact host NTT, the thread fan-out and the key-file codec were each reduced to one copy
(docs/HISTORY.md section 17), so a reorganisation that moves one word, one generator draw or one file byte fails here.

The key-file tests walk all six kinds through every loader.  Sizes against literals, the pair key's payload, the client
and public-key round trips and PublicParameters.save == fhs_client_save_public_key are asserted in test_cabi.py,
test_compressed.py, test_packed.py and test_public_key.py and are not repeated."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_client_kat  # noqa: E402

FHS_ERR_STATE = -3
HEADER_WORDS = (742, 2048, 5, 3, 23, 6)     # lwe_n, poly_n, ks_levels, ks_base_log, pbs_base_log, bsk_quant_bits


@pytest.mark.parametrize("threads", ["1", None])
def test_the_fixture_holds_whatever_the_thread_count(monkeypatch, threads):
    if threads is None:
        monkeypatch.delenv("FHS_CLIENT_THREADS", raising=False)
    else:
        monkeypatch.setenv("FHS_CLIENT_THREADS", threads)
    kat = json.load(open(gen_client_kat.OUT))
    assert (kat["seed"], kat["text"], kat["padding"]) == ("0xF5E57121", "Hello, world", 4)
    got = gen_client_kat.records()
    assert [k for k in kat["arrays"] if got.get(k) != kat["arrays"][k]] == [] and set(got) == set(kat["arrays"])
    assert os.path.getsize(gen_client_kat.OUT) < 10_000


# ---- key files -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(gen_client_kat.SEED)
    yield k
    k.close()


@pytest.fixture(scope="module")
def files(ck, tmp_path_factory):
    """{kind: path} of one file of every kind, written by the C writers"""
    d = tmp_path_factory.mktemp("keyfiles")
    paths = {k: str(d / ("kind%d.key" % k)) for k in range(1, 7)}
    ck.save(paths[1])
    ck.save(paths[2], server_key_only=True)
    ck.save_multibit_key(paths[3])
    ck.save_compressed_server_key(paths[4])
    ck.save_packing_key(paths[5])
    ck.save_public_key(paths[6])
    return paths


@pytest.fixture(scope="module")
def planner():
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    yield sk
    sk.close()


# loader -> the kinds its reader takes
TAKES = {"fhs_client_load": {1}, "fhs_load_server_key_file": {1, 2}, "fhs_load_multibit_key_file": {3},
         "fhs_load_compressed_server_key_file": {4}, "fhs_load_packing_key_file": {5}, "fhs_public_key_load": {6}}


def _reader_accepts(planner, loader, path):
    """Whether the key-file reader behind `loader` took the file.  The context loaders go through a planner context: a
    refused file is FHS_ERR_STATE with the loader's "cannot read ..." text; whatever the call returns after the reader
    (a planner keeps no pair or packing key; a server key wants a device) is not the reader's verdict."""
    import fhestring_amd
    from fhestring_amd.api import MyClientKey, PublicParameters
    L = fhestring_amd.lib()
    if loader in ("fhs_client_load", "fhs_public_key_load"):
        try:
            (MyClientKey if loader == "fhs_client_load" else PublicParameters).load(path).close()
            return True
        except fhestring_amd.FhsError:
            return False
    rc = getattr(L, loader)(planner.ctx._h, path.encode())
    return not (rc == FHS_ERR_STATE and L.fhs_last_error(planner.ctx._h).startswith(b"cannot read"))


def test_headers_sizes_and_payloads(ck, files):
    from fhestring_amd import cabi
    consts = dict(cabi.parse_header()["consts"])
    for kind, name in ((4, "FHS_CKEY_FILE_BYTES"), (5, "FHS_PACK_KEY_FILE_BYTES"), (6, "FHS_PK_FILE_BYTES")):
        assert os.path.getsize(files[kind]) == consts[name], name          # (kinds 1 to 3: test_cabi.py's formulas)
    for kind, path in files.items():
        with open(path, "rb") as f:
            assert f.read(64) == b"FHSKEY01" + struct.pack("<7Q", kind, *HEADER_WORDS), kind
    lwe, glwe = ck.secret_keys()
    seed, bb, kb = ck.compressed_server_key()
    server = [ck.bsk(), ck.ksk()]
    payload = {1: [np.array([gen_client_kat.SEED], np.uint64), lwe, glwe] + server, 2: server, 4: [seed, bb, kb],
               5: [ck.packing_key()]}                                           # (kind 3: test_cabi.py, kind 6: test_public_key.py)
    for kind, arrays in payload.items():
        with open(files[kind], "rb") as f:
            f.seek(64)
            for a in arrays:
                assert f.read(a.nbytes) == a.tobytes(), kind
            assert f.read() == b"", kind


def test_every_reader_takes_its_kinds_and_refuses_the_others(files, planner):
    for loader, kinds in TAKES.items():
        for kind, path in files.items():
            assert _reader_accepts(planner, loader, path) == (kind in kinds), (loader, kind)


def test_truncated_and_extended_files(files, planner):
    """One byte more is refused for kinds 3 to 6 and accepted by both readers of kinds 1 and 2; one byte less is refused by
    every reader.  The first half is the behaviour as found, not a rule of the format: it is pinned here so that a change
    is deliberate."""
    for kind, path in files.items():
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            f.seek(size - 1)
            last = f.read(1)
        loaders = [l for l, kinds in TAKES.items() if kind in kinds]
        try:
            with open(path, "ab") as f:
                f.write(b"\0")
            for loader in loaders:
                assert _reader_accepts(planner, loader, path) == (kind in (1, 2)), (loader, kind, "one byte more")
            os.truncate(path, size - 1)
            for loader in loaders:
                assert not _reader_accepts(planner, loader, path), (loader, kind, "one byte less")
        finally:
            os.truncate(path, size - 1)
            with open(path, "ab") as f:
                f.write(last)
        assert os.path.getsize(path) == size
