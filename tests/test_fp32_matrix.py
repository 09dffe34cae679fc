"""CPU checks of the fp32 kernel matrix (tests/fp32_matrix.py): the table names every fp32 convolution kernel the build produces -- by set equality
with the kernel symbols of the built objects --, every case's layers run the kernel families its keys say (w2xc_layer_kernel_name answers without a
device), and the second-trip sizes really give a workgroup a second item.  tests/test_gpu_fp32_matrix.py launches the cases."""
import os
import sys

import numpy as np
import pytest

import fp32_matrix as fm

PAIRS = [
    ("_Z13conv3x3_wino4ILi128ELi64ELb1ELb0ELb1ELb0EEv12W2xcConvDescii", "void conv3x3_wino4<128, 64, true, false, true, false>(W2xcConvDesc, int, int)",
     ("conv3x3_wino4", (128, 64, True, False, True, False))),
    ("_Z13conv3x3_firstILi3ELi4ELb1ELb1EEv12W2xcConvDescii", "void conv3x3_first<3, 4, true, true>(W2xcConvDesc, int, int)",
     ("conv3x3_first", (3, 4, True, True))),
    ("_Z13conv3x3_mfma2ILi32ELi64ELi2ELi1ELi4ELi2ELi1EEv12W2xcConvDescii", "void conv3x3_mfma2<32, 64, 2, 1, 4, 2, 1>(W2xcConvDesc, int, int)",
     ("conv3x3_mfma2", (32, 64, 2, 1, 4, 2, 1))),
    ("_Z20upconv4x4_head_batchILi256ELi1ELb0EEv12W2xcConvDescii13W2xcBatchDesc", "void upconv4x4_head_batch<256, 1, false>(W2xcConvDesc, int, int, W2xcBatchDesc)",
     ("upconv4x4_head_batch", (256, 1, False))),
    ("_Z21conv3x3_wino4_batch_lILi32ELi128ELb0ELb1EEv12W2xcConvDescii13W2xcBatchDesc",
     "void conv3x3_wino4_batch_l<32, 128, false, true>(W2xcConvDesc, int, int, W2xcBatchDesc)", ("conv3x3_wino4_batch_l", (32, 128, False, True))),
    ("_Z14conv3x3_direct12W2xcConvDesci", "conv3x3_direct(W2xcConvDesc, int)", ("conv3x3_direct", ())),
    ("_Z28conv3x3_last_gather_x4_batchPKfixxxS0_Pfxiixx",
     "conv3x3_last_gather_x4_batch(float const*, int, long long, long long, long long, float const*, float*, long long, int, int, long long, long long)",
     ("conv3x3_last_gather_x4_batch", ())),
]


@pytest.fixture(scope="module")
def built():
    if not all(os.path.exists(os.path.join(fm.LIB, o)) for o in fm.kernel_objects()):
        sys.path.insert(0, fm.ROOT)
        import __graft_entry__ as graft
        graft.build()
    return fm.built_keys()


@pytest.mark.parametrize("symbol,demangled,key", PAIRS, ids=[p[2][0] + "_" + "_".join(str(int(a)) for a in p[2][1]) for p in PAIRS])
def test_key_of_name_reads_both_spellings(symbol, demangled, key):
    assert fm.key_of_name(symbol) == key and fm.key_of_name(demangled) == key
    assert fm.key_of_name(demangled.replace("void ", "")) == key
    assert fm.is_fp32_conv(symbol) and fm.is_fp32_conv(demangled)


def test_names_outside_the_matrix():
    assert not fm.is_fp32_conv("_Z13conv3x3_splitILi32ELi32ELi2ELi1ELi4ELi1ELi1ELi1ELi2ELi3ELi0ELi1EEv12W2xcConvDescii")
    assert not fm.is_fp32_conv("void k_px<U8ToRgb>(U8ToRgb, long long, int)") and not fm.is_fp32_conv("_Z13repack_kernelPKfxxxPfxxxiii")
    assert fm.key_of_name("Cijk_Ailk_Bljk_SB_MT64x64x8") is not None and fm.key_of_name("_Z13conv3x3_wino4ILx5EEv") is None


def test_the_makefile_names_every_kernel_object():
    objs = fm.kernel_objects()
    assert len(objs) == len(set(objs)) >= 26 and "w2xc_wino4_bw.o" in objs and "w2xc_kernels.o" in objs and "w2xc_upconv_b.o" in objs and not any("select" in o or "pack" in o for o in objs)


def test_every_built_symbol_has_a_key(built):
    syms = fm.built_symbols()
    assert len(syms) > 100
    keys = [fm.key_of_name(s) for s in syms]
    assert None not in keys, [s for s, k in zip(syms, keys) if k is None]
    assert len(set(keys)) == len(syms), "two symbols with one key"
    assert built == set(keys)


def test_the_table_covers_exactly_the_built_kernels(built):
    covered = fm.covered_keys()
    missing, unknown = built - covered - set(fm.UNREACHABLE), (covered | set(fm.UNREACHABLE)) - built
    assert not missing, "instantiations without a case: %r" % sorted(missing)
    assert not unknown, "keys of the table that the build does not have: %r" % sorted(unknown)
    assert not covered & set(fm.UNREACHABLE), sorted(covered & set(fm.UNREACHABLE))
    assert covered | set(fm.UNREACHABLE) == built


def test_unreachable_entries_quote_their_condition():
    src = {}
    for key, why in fm.UNREACHABLE.items():
        refs = [r for r in __import__("re").findall(r"(w2xc_\w+\.(?:cpp|hip|hpp|h)):(\d+)", why)]
        assert refs, (key, why)
        quotes = __import__("re").findall(r"`([^`]+)`", why)
        assert quotes, (key, why)
        f, line = refs[0]
        text = src.setdefault(f, open(os.path.join(fm.CSRC, f)).read().splitlines())
        assert any(q in text[int(line) - 1] for q in quotes), (key, f, line, text[int(line) - 1])
    assert 10 * len(fm.UNREACHABLE) <= len(fm.built_symbols()), "more than a tenth of the kernels called unreachable"


def opts_of(w2xc, case, **more):
    return w2xc.make_opts(**dict(case.opts, **more))


@pytest.fixture(scope="module")
def model_sets(w2xc):
    assert (w2xc.KERNEL_AUTO, w2xc.KERNEL_DIRECT, w2xc.KERNEL_MFMA, w2xc.KERNEL_WINOGRAD32) == (fm.KERNEL_AUTO, fm.KERNEL_DIRECT, fm.KERNEL_MFMA, fm.KERNEL_WINOGRAD32)
    assert (w2xc.FUSION_AUTO, w2xc.FUSION_OFF, w2xc.FUSION_PROG) == (fm.FUSION_AUTO, fm.FUSION_OFF, fm.FUSION_PROG)
    sets = {}
    for c in fm.CASES:
        layers, head = fm.model_arrays(c, fm.seed_of(c))
        sets[c.id] = w2xc._ModelSet.from_layers(layers, head=head)
    return sets


@pytest.mark.parametrize("case", fm.CASES, ids=[c.id for c in fm.CASES])
def test_layers_run_the_families_of_the_keys(w2xc, model_sets, case):
    ms = model_sets[case.id]
    assert ms.n_layers == fm.n_layers(case) == len(case.layer_names)
    assert [ms.kernel_name(l, opts_of(w2xc, case)) for l in range(ms.n_layers)] == list(case.layer_names)
    launched = {n for n in case.layer_names if not n.startswith("(")}
    assert {fm.family_of(k[0]) for k in case.keys} == launched, (sorted(case.keys), case.layer_names)
    batch_forms = {k[0].endswith("_batch") or k[0].endswith("_batch_l") for k in case.keys}
    assert len(batch_forms) == 1, "single-image and batch kernels in one case: %r" % sorted(case.keys)
    assert batch_forms == {case.batch > 1 or case.entry == "rgba_u8_tta"}
    assert case.keys <= {k for k in case.keys if fm.is_fp32_conv(k[0])}
    assert all(s in fm.SIZES for s in case.sizes) and (case.entry in fm.FLOAT_SINGLE + fm.FLOAT_BATCH + fm.U8_ENTRIES)
    if case.batch > 1 and case.entry in fm.FLOAT_BATCH:   # the plan says "one launch per layer" for the batch cases (host arithmetic)
        for s in case.sizes:
            h, w = fm.SIZES[s]
            batched, sub = ms.batch_plan(case.planes[0], w, h, opts=opts_of(w2xc, case), up2x=bool(case.head))
            assert batched and sub >= case.batch, (s, batched, sub)


def test_every_key_runs_at_the_two_small_sizes():
    small = {}
    for c in fm.CASES:
        for k in c.keys:
            small.setdefault(k, set()).update(c.sizes)
    for k, sizes in small.items():
        assert "17x33" in sizes and ("1x1" in sizes or (k[0] == "conv3x3_wino4" and k[1][5] and "4x4" in sizes)), (k, sizes)


SECOND = [(c, s) for c in fm.CASES for s in c.sizes if s in fm.SECOND_TRIP]


@pytest.mark.parametrize("case,size", SECOND, ids=["%s-%s" % (c.id, s) for c, s in SECOND])
def test_second_trip_sizes_give_a_workgroup_a_second_item(case, size):
    assert case.focus is not None
    name, items, grid = fm.focus_launch(case, size)
    assert items > grid, (name, items, grid)
    if case.batch > 1:   # ... and a workgroup's run straddles two images: the items of one image are no multiple of the workgroups' share
        assert (items // case.batch) % grid != 0 or name in ("conv3x3_first", "conv3x3_last")


def test_every_body_has_second_trips_at_its_narrowest_and_widest_shape():
    """a body: a kernel, and for conv3x3_wino4 each layout / FUSE7 / PROG variant (they change the item loop's loads, stores and epilogue)"""
    seen = {}
    for c, s in SECOND:
        k, cout = c.focus
        name = c.layer_names[k - 1]
        for key in c.keys:
            if fm.family_of(key[0]) == name and (len(key[1]) < 2 or key[1][1] == cout or name in ("conv3x3_first", "upconv4x4_head")):
                body = (key[0],) + tuple(a for a in key[1][2:] if isinstance(a, bool))
                seen.setdefault(body, set()).add(key[1][:2])
    want = {("conv3x3_mfma2",): {(32, 32), (128, 128)}, ("conv3x3_wino",): {(32, 32), (128, 128)}, ("conv3x3_wino_batch",): {(32, 32), (128, 32)},
            ("conv3x3_first2_wino4",): {()}, ("conv3x3_first2_wino4_batch",): {()},
            ("upconv4x4_head", False): {(32, 3), (256, 3), (32, 1)}, ("upconv4x4_head", True): {(32, 3)}, ("upconv4x4_head_batch", False): {(32, 3), (256, 3)},
            ("conv3x3_wino4_batch", False): {(64, 64), (128, 128)}, ("conv3x3_wino4_batch", True): {(64, 64), (128, 128)},
            ("conv3x3_wino4_batch_l", False, False): {(64, 64), (128, 128)}, ("conv3x3_wino4_batch_l", False, True): {(32, 64), (32, 128)},
            ("conv3x3_wino4_batch_l", True, True): {(32, 64), (32, 128)}}
    for lay, shapes in {(True, False, False, False): {(64, 64), (128, 128)}, (False, False, False, False): {(64, 64), (128, 128)},
                        (True, True, False, False): {(32, 64), (32, 128)}, (False, True, False, False): {(32, 64), (32, 128)},
                        (True, False, True, False): {(64, 64), (128, 128)}, (True, False, True, True): {(64, 64), (128, 128)},
                        (True, True, True, False): {(32, 64), (32, 128)}}.items():
        want[("conv3x3_wino4",) + lay] = shapes
    for body, shapes in want.items():
        assert shapes <= seen.get(body, set()), (body, shapes, seen.get(body))


def test_first_and_last_layers_walk_on_at_17x33():
    """conv3x3_first / conv3x3_last and their batch, PLANAR and U8 forms: one body each (w2xc_first_body.inc, w2xc_last_body.inc), a workgroup walks
    FIRST_TPW = LAST_TPW = 4 consecutive tiles -- at 17x33 every such layer of every case has more tiles than workgroups and more than one workgroup's share
    of 4, so the tile loop goes round again in every instantiation (the uint8 image calls run the same layers at the same extents)"""
    checked = set()
    for c in fm.CASES:
        if "17x33" not in c.sizes:
            continue
        n, (h, w) = fm.n_layers(c), fm.SIZES["17x33"]
        for k, name in enumerate(c.layer_names, 1):
            if name in ("conv3x3_first", "conv3x3_last"):
                items, grid = fm.launch_shape(name, 32, h + 2 * (n - k), w + 2 * (n - k))
                assert items > grid and items > fm.FIRST_TPW, (c.id, name, items, grid)
                checked |= {key for key in c.keys if fm.family_of(key[0]) == name}
    assert checked == {k for k in fm.covered_keys() if fm.family_of(k[0]) in ("conv3x3_first", "conv3x3_last")}


def test_first_and_last_batches_straddle_images_at_17x33():
    """conv3x3_first_batch / conv3x3_last_batch: a workgroup walks 4 consecutive tiles of batch x tiles, image-major -- with a tile count per image
    that is no multiple of 4 a workgroup's run holds tiles of two images"""
    for c in fm.CASES:
        if c.batch > 1 and c.entry in ("planes_batch", "up2x_batch"):
            n, (h, w) = fm.n_layers(c), fm.SIZES["17x33"]
            tiles = [fm.launch_shape("conv3x3_first", 32, h + 2 * (n - k), w + 2 * (n - k))[0] for k in (1, n) if c.layer_names[k - 1] in ("conv3x3_first", "conv3x3_last")]
            assert tiles and all(t % fm.FIRST_TPW != 0 and t * c.batch > fm.FIRST_TPW for t in tiles), (c.id, tiles)


def test_the_float64_restatements_agree_on_a_one_plane_chain(oracle_built):
    """one plane in and out: the oracle's convert_f64 (the reference of those cases) and upconv_ref.chain_z (the reference of the multi-plane chains)"""
    import upconv_ref as ur
    from tools import gen_model
    from oracle import oracle as orc
    layers = gen_model.synth_layers([1, 32, 64, 1], 77)
    x = np.random.default_rng(3).random((1, 9, 13), dtype=np.float32)
    a, b = orc.Oracle(layers).convert_f64(x[0]), ur.chain_z(layers, x, 3).numpy()[0]
    # (they differ at 3e-9 of the range -- the oracle's LeakyReLU slope is the float 0.1f, torch's the double 0.1 --: a twentieth of an fp32 ulp)
    assert a.shape == b.shape == (9, 13) and np.abs(a - b).max() <= 1e-8 * np.abs(a).max()


def test_conditioning_looks_at_the_reference_only(oracle_built):
    seed, layers, head, src, ref = fm.conditioned("w4_f7_64_64", "1x1")
    assert ref.shape == (1, 1, 1) and (seed - fm.seed_of(fm.BY_ID["w4_f7_64_64"])) % 100 == 0
    seed, layers, head, src, ref = fm.conditioned("head_32_3_u8", "17x33")
    assert ref.shape == (3, 34, 66) and src.dtype == np.uint8 and 0.1 <= ((ref > 0) & (ref < 1)).mean()
