"""CPU: pp_jpeg_scan_prepare (csrc/pp_jpeg_host.h), the host's share of the device Huffman decoder: what it accepts and what
it refuses, the bounds of the entropy-coded segment and the tables against the references, a restart-interval file refused
with that word in the reason, and the library called with every refused input."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_huffdec_cases as C  # noqa: E402
import jpeg_huffdec_ref as R  # noqa: E402
import jpeg_ref as J  # noqa: E402
import jpeg_sources as S  # noqa: E402
from make_golden_jpeg import truncations  # noqa: E402


@pytest.fixture(scope="module")
def jpeg(lib_built):
    from probpose_code_amd import jpeg

    return jpeg


def _table_codes(table) -> dict:
    """{bit string: symbol} of a pp_jpeg_huff_table, read back through its own lookup rules."""
    look = np.asarray(table["look"])
    codes = {}
    for prefix, e in enumerate(look):
        if e:
            codes[format(prefix, "09b")[:int(e) >> 8]] = int(e) & 255
    for length in range(10, 17):
        hi = int(table["maxcode"][length])
        if hi < 0:
            continue
        code = hi
        while code >= 0 and 0 <= code + int(table["valoffset"][length]) < 256:
            bits = format(code, f"0{length}b")
            if any(bits[:k] in codes for k in range(1, length)):
                break
            codes[bits] = int(table["vals"][code + int(table["valoffset"][length])])
            code -= 1
    return codes


def test_accepted_files_segment_bounds_and_tables(jpeg):
    table_dtype = np.dtype([("look", "<u2", 512), ("maxcode", "<i4", 18), ("valoffset", "<i4", 18), ("vals", "u1", 256)])
    assert table_dtype.itemsize == jpeg.TABLE_BYTES
    cases = dict(C.corpus())
    for name in ("33x17_420", "37x29_444", "48x64_grey"):
        for layout in ("plain", "fibonacci", "shared_pair_slots_2_3", "slots_3_2_split", "pq1_sof1", "ids_rgb_with_jfif"):
            cases[f"{name}/{layout}"] = S.transcoded(name, layout)
    for name, data in cases.items():
        scan = jpeg.scan_prepare(data)
        ref, parsed = C.prepared(data), J.parse(data)
        info = scan.info
        assert (info.width, info.height, info.ncomp, info.hs, info.vs, info.mcus_x, info.mcus_y, info.restart_interval, info.supported) == \
            (parsed["width"], parsed["height"], parsed["ncomp"], parsed["hs"], parsed["vs"], parsed["mcus_x"], parsed["mcus_y"], 0, 1), name
        assert info.coef_count == J.flat_coefficients(parsed).size, name
        assert np.array_equal(scan.qtables, parsed["qtables"]) and scan.qtables.dtype == np.uint16, name
        start = scan.stream.ctypes.data - np.frombuffer(scan.data, np.uint8).ctypes.data
        assert (start, scan.stream.size) == (ref["offset"], len(ref["stream"])), name
        assert scan.stream.tobytes() == ref["stream"] and scan.data == data, name
        # the segment ends in front of the EOI marker and holds no marker
        assert data[start + scan.stream.size:start + scan.stream.size + 2] == b"\xff\xd9", name
        raw = scan.stream.tobytes()
        assert all(raw[i + 1:i + 2] == b"\x00" for i in range(len(raw)) if raw[i] == 0xFF), name
        tables = scan.tables.view(table_dtype)
        assert len(tables) == 2 * info.ncomp == len(ref["tables"]), name
        for t, want in zip(tables, ref["tables"]):
            assert _table_codes(t) == want, name


def test_refused_files_name_their_cause(jpeg):
    g = J.golden()
    refused = {n: (d, None) for n, d in g["refused"].items()}
    for name in S.REFUSED:
        refused[name] = S.refused(name)
    restart = [n for n in g["names"] if not n.endswith(("_r0", "optimize", "qtables"))]
    assert len(restart) >= 100
    for name in restart[::7] + ["31x50_422", "120x300_420"]:
        data = g["jpg"][name] if name in g["jpg"] else S.source(name)
        assert jpeg.entropy_decode(data).info.restart_interval > 0, name  # the host Huffman decoder keeps these
        refused[name] = (data, "restart")
    for name, data in C.corpus().items():
        if name.startswith(("48x64_420_q75", "17x33_grey_q95")):
            for kind, cut in truncations(data).items():
                refused[f"{name}/{kind}"] = (cut, "EOI" if kind != "last_mcu_eoi" else "")
    refused["empty"] = (b"", "SOI")
    refused["no_soi"] = (b"\x00" * 64, "SOI")
    assert len(refused) >= 30
    for name, (data, word) in refused.items():
        if word == "":  # (the cut file with EOI put back has a whole segment: the device finds that it ends early)
            assert jpeg.scan_prepare(data).stream.size > 0, name
            with pytest.raises(jpeg.JpegUnsupported):
                jpeg.entropy_decode(data)
            continue
        with pytest.raises(jpeg.JpegUnsupported) as e:
            jpeg.scan_prepare(data)
        assert e.value.reason, name
        if word:
            assert word in e.value.reason, (name, e.value.reason)
        # the library itself, with the refused input: the status, the reason in the struct and in pp_last_error
        scan = jpeg._Scan()
        st = jpeg._lib.lib.pp_jpeg_scan_prepare(data, len(data), ctypes.byref(scan))
        assert st == jpeg._lib.PP_ERR_UNSUPPORTED and scan.info.supported == 0, name
        assert scan.info.reason.decode() == e.value.reason and e.value.reason in jpeg._lib.last_error(), name
        assert scan.stream_bytes == 0 and scan.stream_offset == 0, name
        if not word or word != "restart":
            probe_ok = jpeg.probe(data).supported == 1
            if not probe_ok:
                assert jpeg.probe(data).reason.decode() == e.value.reason, name  # everything pp_jpeg_probe refuses, by its reason


def test_null_arguments_and_reentrancy(jpeg):
    lib = jpeg._lib.lib
    scan = jpeg._Scan()
    assert lib.pp_jpeg_scan_prepare(None, 0, ctypes.byref(scan)) == jpeg._lib.PP_ERR_INVALID_ARG
    assert lib.pp_jpeg_scan_prepare(b"\xff\xd8", 2, None) == jpeg._lib.PP_ERR_INVALID_ARG
    from concurrent.futures import ThreadPoolExecutor

    files = list(C.corpus().values())[:32]
    with ThreadPoolExecutor(4) as pool:
        twice = list(pool.map(lambda d: jpeg.scan_prepare(d).stream.tobytes(), files * 2))
    assert twice[:len(files)] == twice[len(files):] == [R.prepare(d)["stream"] for d in files]


def test_scratch_bytes_arguments(jpeg):
    lib = jpeg._lib.lib
    scan = jpeg.scan_prepare(S.source("33x17_420"))
    info = (jpeg.JpegInfo * 2)(scan.info, scan.info)
    one = lib.pp_jpeg_huffman_scratch_bytes(info, (ctypes.c_longlong * 1)(scan.stream.size), 1)
    assert one > 0 and one % 256 == 0
    assert lib.pp_jpeg_huffman_scratch_bytes(info, (ctypes.c_longlong * 2)(scan.stream.size, scan.stream.size), 2) == 2 * one
    assert lib.pp_jpeg_huffman_scratch_bytes(info, (ctypes.c_longlong * 1)(100000), 1) > one
    assert lib.pp_jpeg_huffman_scratch_bytes(info, (ctypes.c_longlong * 1)(0), 0) == 0
    for bad in ((None, (ctypes.c_longlong * 1)(1), 1), (info, None, 1), (info, (ctypes.c_longlong * 1)(-1), 1),
                (info, (ctypes.c_longlong * 1)(1 << 28), 1), (info, (ctypes.c_longlong * 1)(1), -1)):
        assert lib.pp_jpeg_huffman_scratch_bytes(*bad) == jpeg._lib.PP_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        jpeg._sync_passes(0)
    with pytest.raises(ValueError):
        jpeg._sync_passes(jpeg.MAX_SYNC_PASSES + 1)
