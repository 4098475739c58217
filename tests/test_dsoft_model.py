"""CPU suite of the D-SOFT filter's edge cases (tests/dsoft_cases.py), no GPU touched.  For every case:

* the model (tests/dsoft_model.py) equals the reference's own SeedPosTable::DSOFT + decode (`reflib`: oracle/_ref
  where it is built, else its recorded answers), candidate by candidate and in order;
* the host restatement (darwin-gpu_amd/host/dsoft.cpp through `darwin_hip --dsoft-only --dump-candidates`, every
  parameter in params.cfg) equals the same list;
* the model's trace shows that the case reaches the path it is there for.

Where the reference's own answer is not defined, model and host are held to each other instead (the device as well,
tests/test_gpu_dsoft_edges.py), strand by strand (dsoft_cases.expected).  Three such places are reached here:

* a hit at or past the padded length (`padding`): the reference stops at assert(hit < ref_size_)
  (seed_pos_table.cpp:134); built without assertions it looks up bin_to_chr_id, a std::map, at a bin no sequence owns
  (darwin.cpp:217,256), which inserts sequence 0 from several threads at once.  Model, host and device say sequence 0.
* max_candidates reached on a bin's first hit (`max_candidates_first_hit`): the `break` (seed_pos_table.cpp:145-147)
  leaves the hit loop after the bin was written (:141) and before it is listed for clearing (:150-153), so the next
  query of the same thread starts with that bin counted.  Model, host and device start every strand from clean bins and
  keep the first max_candidates emissions.
* a query of fewer than k + w bases in whole words (`lengths_end255`, k + w = 17, reads of 16 bases and fewer): the
  loop bound 16 * s_len - k - w is unsigned and wraps (ntcoding.cpp:168).  Model, host and device emit nothing.
"""
import struct
import subprocess

import pytest

import dsoft_cases


def host_list(tmp_path, c, threads=2):
    """the driver's per-read order (forward, then reverse complement) put strand-major"""
    from gact_amd import engine
    drv = engine.build_driver()
    lines = []
    for n, r in enumerate(c.reads):
        b = r.decode()
        lines += [">r%d" % n] + [b[k:k + 70] for k in range(0, len(b), 70)]
    (tmp_path / "reads.fasta").write_text("\n".join(lines) + "\n")
    (tmp_path / "params.cfg").write_text("[DSOFT_params]\n" + "".join("%s = %d\n" % kv for kv in sorted(c.params.items())))
    out = subprocess.run([drv, "reads.fasta", "reads.fasta", str(threads), "--dsoft-only", "--dump-candidates", "c.bin"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "c.bin", "rb").read()
    got = [struct.unpack_from("<5i", raw, k) for k in range(0, len(raw), 20)]
    return [x for x in got if x[4] == 0] + [x for x in got if x[4] == 1]


@pytest.mark.parametrize("name", dsoft_cases.NAMES)
def test_model_equals_reference(reflib, name):
    c = dsoft_cases.case(name)
    want = dsoft_cases.expected(reflib, c)
    assert len(want) > 0
    assert c.model()[0] == want


@pytest.mark.parametrize("name", dsoft_cases.NAMES)
def test_host_restatement_equals_reference(reflib, tmp_path, name):
    c = dsoft_cases.case(name)
    assert host_list(tmp_path, c) == dsoft_cases.expected(reflib, c)


def test_host_restatement_is_independent_of_the_thread_split(tmp_path):
    """one thread takes every strand in turn: a bin left counted by a strand would show in the next"""
    c = dsoft_cases.case("max_candidates_first_hit")
    assert host_list(tmp_path, c, threads=1) == c.model()[0]


def test_cases_hold_every_read_on_both_strands_and_itself():
    for name in dsoft_cases.NAMES:
        c = dsoft_cases.case(name)
        lst = c.model()[0]
        assert {x[4] for x in lst} == {0, 1}, name
        assert any(x[0] == x[1] and x[4] == 0 for x in lst), name        # a read against itself (same_file)
        assert c.params["seed_size"] <= 12 and c.band_slots() <= 32768, name
        assert 1000 < sum(map(len, c.reads)) < 140000, name


# ---- reachability: what the model's trace must show, case by case

def hits_of(c):
    return [h for t in c.traces() for h in t.seed_hits]


def boundaries_of(c):
    return [same for t in c.traces() for _, _, same in t.group_boundaries]


@pytest.mark.parametrize("name", ["many_hits_bin64", "many_hits_bin4096"])
def test_many_hits_reaches_the_second_and_third_group_of_64(name):
    c = dsoft_cases.case(name)
    assert c.params["seed_size"] == 8 and c.ref_len() >= 131072 and c.max_occ() >= 96
    assert any(65 <= h <= 128 for h in hits_of(c)) and any(h > 128 for h in hits_of(c))
    assert any(boundaries_of(c)) and not all(boundaries_of(c))      # one bin on both sides; two bins
    assert sum(t.late_emissions for t in c.traces()) > 0             # candidates from hits beyond a seed's first 64


def test_many_hits_carries_a_bin_across_groups_at_both_bin_sizes():
    same64, same4096 = (sum(boundaries_of(dsoft_cases.case(n))) for n in ("many_hits_bin64", "many_hits_bin4096"))
    diff64, diff4096 = (sum(not b for b in boundaries_of(dsoft_cases.case(n))) for n in ("many_hits_bin64", "many_hits_bin4096"))
    assert same64 and diff64 and same4096 and diff4096


@pytest.mark.parametrize("name,threshold", [("low_threshold_eq_k", 10), ("low_threshold_below_k", 7), ("low_threshold_1", 1)])
def test_low_threshold_crosses_on_first_hits(name, threshold):
    c = dsoft_cases.case(name)
    assert c.params["threshold"] == threshold <= c.params["seed_size"] == 10
    n_first = sum(len(t.first_hit_crossings) for t in c.traces())
    assert n_first > 0 and n_first == len(c.model()[0])             # no other way to cross at threshold <= k


def test_full_counter_comes_within_15_of_the_8_bit_limit():
    c = dsoft_cases.case("full_counter")
    assert c.params["threshold"] + c.params["seed_size"] == 255
    assert max(t.max_counter for t in c.traces()) >= 240
    assert len(c.model()[0]) >= 1


def test_padding_reaches_padding_hits_the_clamp_and_the_positions_past_the_end():
    c = dsoft_cases.case("padding")
    assert c.params["seed_size"] + c.params["window_size"] < 16
    assert all(len(r) % c.params["bin_size"] for r in c.reads)
    tr = c.traces()
    assert any(t.padding for t in tr) and any(t.clamped for t in tr) and any(t.past_end for t in tr)
    assert 128 < max(hits_of(c)) <= c.params["seed_occurence_multiple"]      # the all-A seed: three groups, under the cap
    assert all(t.undefined for t in tr if t.past_end)


def test_padding_k12_is_defined_by_the_reference_throughout():
    c = dsoft_cases.case("padding_k12")
    tr = c.traces()
    assert c.params["seed_size"] + c.params["window_size"] == 16
    assert any(t.padding for t in tr) and any(t.clamped for t in tr)
    assert not any(t.past_end or t.undefined for t in tr)


def test_seed_cut_falls_where_each_case_says():
    cut = {n: dsoft_cases.case(n).model()[1][0].cut_at for n in dsoft_cases.NAMES if n.startswith("seed_cut")}
    used = {n: len(dsoft_cases.case(n).model()[1][0].seed_offsets) for n in cut}
    assert used["seed_cut_0"] == 1 and used["seed_cut_1"] == 2
    offset, chunk, number, last = cut["seed_cut_last_of_chunk"]
    assert last and number > 0
    offset2, chunk2, number2, _ = cut["seed_cut_first_of_next"]
    assert chunk2 == chunk + 1 and number2 == 0 and offset2 > offset
    assert used["seed_cut_first_of_next"] == used["seed_cut_last_of_chunk"] + 1


def with_num_seeds(c, num_seeds):
    """read 0's forward list, and the whole list, of the case's reads with another num_seeds"""
    m = dsoft_cases.Case("probe", c.reads, **dict(c.params, num_seeds=num_seeds)).model()
    return m[3][0], m[0]


@pytest.mark.parametrize("name", ["seed_cut_0", "seed_cut_1", "seed_cut_last_of_chunk", "seed_cut_first_of_next"])
def test_seed_cut_one_seed_more_or_fewer_gives_another_list(name):
    """the seed on either side of the cut crosses a bin of its own (dsoft_cases.stairs), so a filter that applies one
    seed too many or too few gives another list for read 0's forward strand, the strand the cut was chosen on"""
    c = dsoft_cases.case(name)
    n = c.params["num_seeds"]
    here, more = with_num_seeds(c, n), with_num_seeds(c, n + 1)
    assert here == (c.model()[3][0], c.model()[0])
    assert more[0][:len(here[0])] == here[0] and len(more[0]) > len(here[0]) and more[1] != here[1]
    if n > 0:
        fewer = with_num_seeds(c, n - 1)
        assert here[0][:len(fewer[0])] == fewer[0] and len(here[0]) > len(fewer[0]) and fewer[1] != here[1]
    # the candidates that one seed more adds lie at the refused seed's position
    assert {x[2] for x in more[0][len(here[0]):]} == {c.model()[1][0].cut_at[0]}


def test_seed_cut_chunk_edge_cases_differ():
    a, b = (dsoft_cases.case(n) for n in ("seed_cut_last_of_chunk", "seed_cut_first_of_next"))
    assert a.reads == b.reads and b.params["num_seeds"] == a.params["num_seeds"] + 1
    assert a.model()[3][0] != b.model()[3][0] and a.model()[0] != b.model()[0]


@pytest.mark.parametrize("name,end", [("lengths_end255", 255), ("lengths_end256", 256), ("lengths_end257", 257)])
def test_lengths_stand_on_both_sides_of_every_boundary(name, end):
    c = dsoft_cases.case(name)
    k, w = c.params["seed_size"], c.params["window_size"]
    lens = {len(r) for r in c.reads}
    assert {k + w - 1, k + w, k + w + 1, 15, 16, 17, 31, 32, 33, 1} <= lens
    undefined = [q for q, t in enumerate(c.model()[1]) if t.undefined]
    assert all(16 * ((len(c.reads[q]) + 15) // 16) < k + w for q in undefined)
    assert bool(undefined) == (k + w > 16)
    # both reads scanned to `end`, one of whole words and one that ends inside its last word, have on either strand a
    # candidate at the last scanned position, from a bin that only the seed there meets: a scan that ends one position
    # early, or never runs a chunk of one position (end = 257), loses it
    _, _, _, forward, reverse = c.model()
    at_end = [q for q, r in enumerate(c.reads) if dsoft_cases.scanned(len(r), k, w) == end]
    assert sorted(len(c.reads[q]) % 16 == 0 for q in at_end) == [False, True]
    stairs_read = len(c.reads) - 1
    for q in at_end:
        for cands in (forward[q], reverse[q]):
            last = [x for x in cands if x[2] == end - 1]
            assert len(last) == 1 and last[0][0] == stairs_read
            assert max(x[2] for x in cands) == end - 1


def test_lengths_cover_255_256_and_257_scanned_positions():
    got = set()
    for name in ("lengths_end255", "lengths_end256", "lengths_end257"):
        c = dsoft_cases.case(name)
        k, w = c.params["seed_size"], c.params["window_size"]
        got |= {16 * ((len(r) + 15) // 16) - k - w for r in c.reads}
    assert {255, 256, 257} <= got


def test_windows_cover_the_smallest_and_largest_window_and_bin():
    p = {n: dsoft_cases.case(n).params for n in dsoft_cases.NAMES if n.startswith("windows")}
    assert p["windows_w1"]["window_size"] == 1
    assert p["windows_wk1"]["window_size"] == p["windows_wk1"]["seed_size"] - 1
    assert p["windows_bin1"]["bin_size"] == 1 and p["windows_bin48"]["bin_size"] == 48
    c = dsoft_cases.case("windows_bin_over_reads")
    assert c.params["bin_size"] > max(map(len, c.reads))


def test_max_candidates_cuts_and_only_the_first_hit_case_is_undefined():
    c = dsoft_cases.case("max_candidates")
    assert any(t.n_emitted > c.params["max_candidates"] for t in c.traces())
    assert not any(t.undefined for t in c.traces())
    c = dsoft_cases.case("max_candidates_first_hit")
    assert c.params["threshold"] <= c.params["seed_size"]
    assert any(t.undefined for t in c.traces())
