"""Every plain-C client under tests/cabi/ compiles as C11 without a warning against include/ and the HIP runtime's headers: compiled,
not linked, so neither libgsr_hip.so nor a GPU is asked for.  The clients are found by name, so a new one is covered as it arrives."""
import glob
import os
import subprocess

import pytest

from tests import cabi_client as cc

CLIENTS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(cc.CABI, "*_client.c")))


def test_the_clients_are_found():
    assert "c_client.c" in CLIENTS and len(CLIENTS) >= 10, CLIENTS


@pytest.mark.parametrize("name", CLIENTS)
def test_client_compiles_without_warnings(name, tmp_path):
    r = subprocess.run([cc.CC, "-std=c11", "-O1", "-Wall", "-Werror", "-c", os.path.join(cc.CABI, name), *cc.INCLUDES, "-o", str(tmp_path / "client.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
