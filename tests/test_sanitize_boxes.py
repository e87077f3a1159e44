"""CPU: the metadata extractor of the box targets (aeon_amd/csrc/box_host.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer.  `make -C aeon_amd/csrc sanitize_boxes` builds tests/sanitize/box_driver.cpp
(a stand-alone program over box_host.cpp alone); it runs over a corpus this test writes: aeon's three VOC
files, truncations of one at every 37th byte, missing keys, a string where a number belongs, 10 000
objects, nesting 10 000 deep and an empty file.  The run must end clean: valid files report aeon's box
counts, the others an error code."""
import json
import os
import subprocess

import pytest

from tests import box_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "box_driver")
VOC_DIR = os.path.join(ROOT, "tests", "golden", "voc")


def _corpus(d):
    files = {}
    for name in sorted(C.VOC):
        files["voc_" + name] = open(os.path.join(VOC_DIR, name), "rb").read()
    whole = files["voc_006637.json"]
    for cut in range(0, len(whole), 37):
        files[f"trunc_{cut:05d}.json"] = whole[:cut]
    base = json.loads(whole)
    for key in ("object", "size"):
        j = dict(base)
        del j[key]
        files[f"missing_{key}.json"] = json.dumps(j).encode()
    for key in ("width", "height", "depth"):
        j = json.loads(whole)
        del j["size"][key]
        files[f"missing_size_{key}.json"] = json.dumps(j).encode()
    for key in ("xmin", "ymin", "xmax", "ymax"):
        j = json.loads(whole)
        del j["object"][2]["bndbox"][key]
        files[f"missing_{key}.json"] = json.dumps(j).encode()
    for key in ("bndbox", "name"):
        j = json.loads(whole)
        del j["object"][5][key]
        files[f"missing_object_{key}.json"] = json.dumps(j).encode()
    j = json.loads(whole)
    j["object"][1]["bndbox"]["xmax"] = "365"
    files["string_for_number.json"] = json.dumps(j).encode()
    j = json.loads(whole)
    j["size"]["width"] = "500"
    files["string_for_width.json"] = json.dumps(j).encode()
    j = json.loads(whole)
    j["size"]["height"] = 1e300
    files["huge_height.json"] = json.dumps(j).encode()
    j = json.loads(whole)
    j["object"][0]["difficult"] = "no"
    files["string_for_bool.json"] = json.dumps(j).encode()
    j = json.loads(whole)
    j["object"] = [dict(base["object"][i % 6], bndbox={"xmin": i, "ymin": i + 1, "xmax": i + 2, "ymax": i + 3})
                   for i in range(10000)]
    files["many_objects.json"] = json.dumps(j).encode()
    files["deep_arrays.json"] = b"[" * 10000 + b"]" * 10000
    files["deep_objects.json"] = b'{"object":' * 10000 + b"1" + b"}" * 10000
    files["deep_in_object.json"] = whole.rstrip()[:-1] + b', "x": ' + b"[" * 10000 + b"]" * 10000 + b"}"
    files["empty.json"] = b""
    files["not_json.json"] = b"\x00\xff\xfe garbage"
    files["object_not_list.json"] = json.dumps(dict(base, object=7)).encode()
    for k, v in files.items():
        (d / k).write_bytes(v)
    return files


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_boxes"])
    d = tmp_path_factory.mktemp("boxes")
    files = _corpus(d)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([DRIVER, json.dumps(C.LABEL_LIST)] + [str(d / k) for k in sorted(files)], capture_output=True,
                       text=True, env=env, timeout=300)
    results = {}
    for line in r.stdout.splitlines():
        path, res = line.split("\t", 1)
        results[os.path.basename(path)] = res
    return r, results, files


def test_runs_clean(run):
    r, results, files = run
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert set(results) == set(files)
    for k, res in results.items():
        assert res.startswith("ok ") or res.startswith("error -1 "), (k, res)


def test_valid_files_report_aeons_counts(run):
    _, results, _ = run
    assert results["voc_000001.json"].startswith("ok 353x500x3 boxes 2 ")
    assert results["voc_000001.json"].endswith("labels 1,0")
    assert results["voc_006637.json"].startswith("ok 500x375x3 boxes 6 ")
    assert results["voc_009952.json"].split(" boxes ")[1].startswith("1 ")
    assert results["many_objects.json"].startswith("ok 500x375x3 boxes 10000 ")
    assert results["deep_in_object.json"] == "error -1 json: nesting too deep"


def test_malformed_files_report_errors(run):
    _, results, files = run
    for k in files:
        if k.startswith("voc_") or k == "many_objects.json":
            continue
        assert results[k].startswith("error -1 "), (k, results[k])
    assert results["deep_arrays.json"] == results["deep_objects.json"] == "error -1 json: nesting too deep"
    assert results["missing_object.json"] == "error -1 'object' missing from metadata"
    assert results["missing_xmax.json"] == "error -1 'xmax' missing from metadata"
    assert results["missing_object_bndbox.json"] == "error -1 'xmax' missing from metadata"
    assert results["missing_size_depth.json"] == "error -1 'depth' missing from metadata"
    assert results["empty.json"].startswith("error -1 json:")
    assert sum(k.startswith("trunc_") for k in files) > 30
