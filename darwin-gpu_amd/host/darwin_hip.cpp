// darwin_hip.cpp -- a darwin.cpp-shaped driver around the GACT shim.
//
//   darwin_hip <REF.fasta> <READS.fasta> CPU_THREADS [--params params.cfg]
//              [--candidates FILE | --dump-candidates FILE [--dsoft-only]] [--device-dsoft]
//              [--device D] [--shard R/W] [--recode] [--cigar] [--paf] [--unique exact|pair] [--coverage K]
//              [--pileup K [--ins-slots S] [--vcf A:P:H]] [--gfa [--unitigs K [--bubbles D] [--clean LO:HI:N]]] [--sam primary|all]
//              [--min-identity P[:S[:D]]]
//
// Plays the part of reference darwin.cpp:451-646 for the GACT stage: owns the
// globals gact.cpp reads, loads params.cfg and the two FASTA files, builds the
// reverse complements (darwin.cpp:110-147), GPU_init, fans candidates out over
// feeder threads (contiguous ranges, darwin.cpp:619-629), each thread calling
// GACT_Batch for its forward and then its reverse-complement calls
// (darwin.cpp:429-433) into darwin.<thread>.out, GPU_close.
//
// Candidates come from the D-SOFT restatement (dsoft.cpp; darwin.cpp:209-288 per read:
// forward strand, then reverse complement) or, with --candidates, from FILE: int32
// records {ref_id, query_id, ref_pos, query_pos, comp}.  --dump-candidates writes the
// same format; --dsoft-only stops after the filter (no GPU is touched).
// --device-dsoft runs the filter on the GPU as well (gact_hip_dsoft_build / _query): every feeder thread
// filters its read range straight into its slot's device candidate array and extends it from there.
// --cigar (with --device-dsoft): every line gets ", cigar: <CIGAR>" appended, the alignment of that overlap from a second
// pass over the emitted candidates (gact_hip_candidates_paths; '=' / 'X' / 'I' / 'D' relative to the reference).
// --paf (with --device-dsoft): every feeder also writes darwin.<thread>.paf beside its unchanged .out file, one PAF line per
// emitted overlap that has an alignment, in the .out file's order -- matches, block length and the span the alignment covers
// from the device's summaries of the emitted candidates (gact_hip_candidates_summaries, gact_hip_format_paf).  With --cigar
// as well each PAF line carries cg:Z:<CIGAR>.
// --unique exact|pair (with --device-dsoft, not with --shard): every feeder selects among its run's records on the device
// (gact_hip_select_overlaps) -- exact: each line once, what `sort | uniq` of its file would leave; pair: one line per (ref, query,
// strand), the overlap with the highest score, then the longer one, then the earlier one.  The .out file keeps its order and
// gets the selected lines only, and --cigar / --paf make their second pass over the selected records only.
// --coverage K (with --device-dsoft, not with --shard; K >= 1): after the feeders have finished, the records they wrote (the
// emitted ones; with --unique the selected ones) go through one gact_hip_read_coverage call, and darwin.cover.tsv gets one line
// per sequence in id order: name, len, n_intervals, max_depth, covered, well_covered (depth >= K), span_begin, span_end (the
// longest stretch that is covered K deep) and mean_depth, tab-separated.  Same file: both sides of every record over the
// reads; different files: the ref side over the reference sequences.  With --paf the summaries go along, so the table is what
// the .paf files' own columns give.  Every other output byte is as without the flag.
// --pileup K (with --device-dsoft, not with --shard; K >= 1): the alignments of the records the feeders write (the emitted ones;
// with --unique the selected ones) are stacked on their target sequences on the device -- gact_hip_pileup_begin over all of
// them before the feeders start, one gact_hip_pileup_add per feeder behind its run, gact_hip_pileup_finish(K) after the join --
// and darwin.cons.fa gets one record per reference sequence in id order: `>name called=<n> changed=<n> deleted=<n>
// ins_flagged=<n>`, then the consensus bytes with every '-' left out, on one line.  Every other output byte is as without the flag.
// --ins-slots S (with --pileup; 1 <= S <= 4): the window is opened with S slots (gact_hip_pileup_begin_ins), so the adds keep the
// first S bases of every insertion run, and darwin.cons.fa gets the corrected reads of gact_hip_pileup_corrected(K) -- the bases
// the other reads agree the sequence lacks put in, the header line with ` inserted=<n>` at its end.  Every other file is as
// without the flag, and without it darwin.cons.fa is too.
// --gfa (with --device-dsoft and one input file used for both sides, not with --shard): after the feeders have finished, the
// records they wrote (the emitted ones; with --unique the selected ones; with --paf together with their summaries) go through
// one gact_hip_overlap_graph call with the default parameters -- with --coverage K clipped to that table's spans, else against
// whole reads -- and darwin.gfa gets `H VN:Z:1.0`, one `S <name> <clipped bases> LN:i:<n>` line per read that is not contained
// and has a non-empty clip, in id order, and one `L <u name> <+|-> <v name> <+|-> <min(ov_u, ov_v)>M L1:i:<len>` line per kept
// arc, in the arc list's order.  Every other output byte is as without the flag.
// --unitigs K (with --gfa; K >= 0): behind the graph call one gact_hip_unitigs call with tip_reads = K and bases, over the same
// lengths, clip, reads and arcs, and darwin.utg.gfa gets `H VN:Z:1.0`; per unitig, numbered from 1 in the call's order, one
// `S utg<6 digits><l|c> <bases> LN:i:<length>` line (l linear, c circular) followed by one `a <utg> <start> <read name>:<b>-<e>
// <+|-> <take>` line per entry of its layout, [b, e) the read's clip; and then one `L <utg> <+|-> <utg> <+|-> <min(ov_u, ov_v)>M`
// line per link (include/gact_hip.h, rule 7), in the arc list's order.  Every other output byte is as without the flag.
// --bubbles D (with --gfa --unitigs K, K >= 1; 1 <= D <= 2^30): behind the graph call one gact_hip_unitigs call without bases to
// learn the tips, then gact_hip_pop_bubbles with those tips as skip and max_dist = D; darwin.bubbles.tsv gets one line per
// bubble found: source, sink, state (0 popped, 1 lost), n_vertices, n_path, n_removed, path_len, tab-separated; and the unitig
// call of --unitigs runs over the arcs with arc_flags written into their flags -- its tip cut is the second round -- so
// darwin.utg.gfa is made from the cleaned arcs.  darwin.gfa and every other file are as without the flag.
// --clean LO:HI:N (with --gfa --unitigs K, K >= 1; integers, 0 <= LO <= HI <= 1000 per mille, 0 <= N <= 16 ratios): behind the graph
// call one gact_hip_clean_graph call with tip_reads = K, max_dist = D of --bubbles (which then only supplies it; without it the
// default) and the ratios LO .. HI in N steps; darwin.clean.tsv gets one line per step of its log: index, kind (tips, bubbles or
// prune), param, reads_removed, examined, arcs_removed, arcs_left, tab-separated; darwin.bubbles.tsv is not written; and the
// unitig call of --unitigs runs over the arcs with arc_flags written into their flags.  Every other file is as without the flag.
// --sam primary|all (with --device-dsoft, not with --shard): every feeder places its reads on the device behind its run (and
// behind --unique) -- the summaries of the records it writes, gact_hip_place_reads over the slot's own records and the window
// of its reads, gact_hip_candidates_paths for the records to print -- and writes darwin.<thread>.sam, a SAM file of its own:
// `@HD VN:1.6 SO:unsorted`, one `@SQ SN:<name> LN:<n>` per reference sequence in id order, `@PG ID:darwin_hip`, then per read in
// id order its primary and supplementary lines (all: its secondary and extra lines too) in rank order, or one unmapped line
// (gact_hip_format_sam, gact_hip_format_sam_unmapped).  Every other output byte is as without the flag.
// --vcf A:P:H (with --pileup K; integers min_alt:min_permille:hom_permille, A >= 1, 0 <= P <= H <= 1000; min_depth is K): after
// the join, behind darwin.cons.fa, one gact_hip_pileup_variants call over the same counts and darwin.vcf: `##fileformat=VCFv4.2`,
// one `##contig=<ID=name,length=n>` per reference sequence, the INFO lines of DP and AD and the FORMAT line of GT, the
// `#CHROM ... FORMAT darwin` line, then the records in device order (gact_hip_format_vcf).  A stated rule of thresholds: no QUAL,
// no likelihoods.  With --sam as well a feeder's gact_hip_pileup_add takes only the records its placement made primary or
// supplementary -- the one gact_hip_place_reads call serves both -- so that a read that maps onto several copies of a repeat
// votes once, and darwin.cons.fa is made from those counts too.  Without --vcf every output byte is as without the flag.
// --min-identity P[:S[:D]] (with --device-dsoft, not with --rccl-gather; integers, 0 <= P <= 1000 per mille, S >= 0 bases,
// 0 <= D <= 1000 per mille): every feeder, behind its run and behind --unique, takes the summaries of the records it would write
// (one gact_hip_candidates_summaries call, which serves --paf as well) and filters them on the device (gact_hip_filter_overlaps):
// a record goes when its alignment has no column, when its identity -- matches per mille of its columns -- is under P, when the
// shorter of its two spans is under S, or, with a D, when it lies more than D under the best record of its query read (the
// feeder's own reads are the window: a feeder holds every record of its reads).  Everything behind it -- the .out lines,
// --cigar, --paf, --coverage, --gfa, --pileup, --sam -- sees the kept records only, and stdout gets one line per feeder: kept of
// counted, and the dropped ones per reason.  A malformed value is refused before any file is read.  Without the flag every output
// byte is as before.
//
// --device D: the GPU this process uses (the reference is single-device, cuda_host.cu:195).  --shard R/W: this
// process is rank R of W -- it extends every W-th candidate (host filter) or the R-th contiguous range of reads
// (--device-dsoft) and writes darwin.<R>.<thread>.out; the union of all ranks' files is the W = 1 output, and the
// reference's canonical form `cat darwin.*.out | sort | uniq` (README:25) is the gather.  --recode: hand the
// read sets to GACT_Batch the way the reference's -DGPU build does, recoded in place to A0 C1 T2 G3
// (darwin.cpp:314-398).  Stage timers are printed with the reference's labels (darwin.cpp:300,405,441,553-639).
//
//   darwin_hip --selftest FILE   exercises AlignWithBT / Align_Batch / Align_Batch_GPU / GACT
//                                on the cases in FILE and prints what they return.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <chrono>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "align.h"
#include "dsoft.h"
#include "gact.h"
#include "gact_hip.h"

// ---- the globals of darwin.cpp:39-93 that gact.cpp / the shim read
bool same_file = false;
int NUM_BLOCKS = 32, THREADS_PER_BLOCK = 64, BATCH_SIZE = 2048;
int match_score = 1, mismatch_score = -1, gap_open = -1, gap_extend = -1;
int first_tile_score_threshold = 35;
int tile_size = 320, tile_overlap = 120;
int num_threads = 1;
static bool want_cigar = false;                  // --cigar
static bool want_paf = false;                    // --paf
static int unique_mode = -1;                     // --unique: GACT_SELECT_EXACT / GACT_SELECT_PAIR, -1: every emitted record
static int coverage_depth = 0;                   // --coverage K: min_depth of darwin.cover.tsv, 0: no table
static int pileup_depth = 0;                     // --pileup K: min_depth of darwin.cons.fa, 0: no consensus
static int pileup_ins_slots = 0;                 // --ins-slots S: the inserted bases kept per position, 0: none
static bool want_gfa = false;                    // --gfa: darwin.gfa, the overlap graph of the records written
static int unitig_tips = -1;                     // --unitigs K: tip_reads of darwin.utg.gfa, -1: no unitigs
static bool want_vcf = false;                    // --vcf A:P:H: darwin.vcf from the pileup's counts (min_depth is --pileup's K)
static int vcf_min_alt = 0, vcf_min_permille = 0, vcf_hom_permille = 0;
static int sam_mode = 0;                         // --sam: 1 primary (and supplementary) lines, 2 all lines, 0: no SAM files
static int clean_lo = -1, clean_hi = 0, clean_n = 0;   // --clean LO:HI:N: the ratios of the cleaning rounds in front of the unitigs, lo < 0: none
static int bubble_dist = 0;                      // --bubbles D: max_dist of the bubble popping in front of the unitigs, 0: none
static bool want_filter = false;                 // --min-identity P[:S[:D]]: the records filtered on the device behind --unique
static gact_filter_params filter_params = {0, GACT_FILTER_DEFAULT_MIN_SPAN, GACT_FILTER_DEFAULT_MAX_DROP_PERMILLE};
static bool filter_relative = false;             // ... with a D: the relative rule over the feeder's own reads
// --coverage, --gfa: the records every feeder wrote a line for, in its file's order, and with --paf their summaries
static std::vector<std::vector<gact_overlap> > cover_records;
static std::vector<std::vector<gact_path_summary> > cover_sums;
std::vector<long long int> reference_lengths, reads_lengths;
std::vector<std::string> reference_seqs, reads_seqs, rev_reads_seqs;
std::vector<std::vector<std::string> > reference_descrips, reads_descrips;

static std::string rev_comp(const std::string &seq)
{
    std::string rc;
    rc.reserve(seq.size());
    for (size_t k = seq.size(); k-- > 0;) {
        switch (seq[k]) {                       // darwin.cpp:122-142
            case 'a': rc += 't'; break; case 'A': rc += 'T'; break;
            case 'c': rc += 'g'; break; case 'C': rc += 'G'; break;
            case 'g': rc += 'c'; break; case 'G': rc += 'C'; break;
            case 't': rc += 'a'; break; case 'T': rc += 'A'; break;
            case 'n': rc += 'n'; break; case 'N': rc += 'N'; break;
            default: std::cerr << "Bad Nt char: " << seq[k] << std::endl; exit(1);
        }
    }
    return rc;
}

// header fields split on anything but [A-Za-z0-9_] (fasta.cpp:19-33); field 0 is the printed name
static std::vector<std::string> split_header(const std::string &h)
{
    std::vector<std::string> out;
    std::string cur;
    for (char c : h) {
        const bool ok = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_';
        if (ok) cur += c;
        else if (!cur.empty()) { out.push_back(cur); cur.clear(); }
    }
    if (!cur.empty()) out.push_back(cur);
    if (out.empty()) out.push_back("");
    return out;
}

static void parse_fasta(const std::string &path, std::vector<std::vector<std::string> > &descrips,
                        std::vector<std::string> &seqs, std::vector<long long int> &lengths)
{
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(1); }
    std::string line, cur;
    bool have = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') {
            if (have) { seqs.push_back(cur); lengths.push_back((long long)cur.size()); }
            descrips.push_back(split_header(line.substr(1)));
            cur.clear(); have = true;
        } else if (have) {
            cur += line;
        }
    }
    if (have) { seqs.push_back(cur); lengths.push_back((long long)cur.size()); }
}

// [section] key = value, '#' / ';' comments (ConfigFile.cpp:30-56); values through atof (Chameleon.cpp:89-91)
static std::map<std::string, double> parse_cfg(const std::string &path)
{
    std::map<std::string, double> kv;
    std::ifstream in(path);
    std::string line, section;
    while (std::getline(in, line)) {
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        if (line[a] == '#' || line[a] == ';') continue;
        if (line[a] == '[') { section = line.substr(a + 1, line.find(']') - a - 1); continue; }
        const size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        std::string key = line.substr(a, eq - a), val = line.substr(eq + 1);
        key.erase(key.find_last_not_of(" \t") + 1);
        kv[section + "/" + key] = atof(val.c_str());
    }
    return kv;
}

struct Cand { int ref_id, query_id, ref_pos, query_pos, comp; };

// ---- stage timers with the reference's labels (darwin.cpp:300,405,441 per thread; :553,574,596,639 in main)
static std::mutex io_lock;
typedef std::chrono::steady_clock::time_point Tick;
static Tick now() { return std::chrono::steady_clock::now(); }
static void print_stage(const char *label, Tick a, Tick b)
{
    const long ms = (long)(std::chrono::duration<double, std::milli>(b - a).count() + 0.5);
    std::lock_guard<std::mutex> lk(io_lock);
    std::cout << label << ": " << ms << " msec" << std::endl;
}

static int shard_rank = 0, shard_world = 1;
static std::string out_name(int cpu_id)
{
    // darwin.cpp:174; ranks of a sharded run keep their files apart
    return shard_world > 1 ? "darwin." + std::to_string(shard_rank) + "." + std::to_string(cpu_id) + ".out"
                           : "darwin." + std::to_string(cpu_id) + ".out";
}

// --paf: darwin.<thread>.paf beside darwin.<thread>.out
static std::string paf_name(int cpu_id)
{
    const std::string out = out_name(cpu_id);
    return out.substr(0, out.size() - 3) + "paf";
}

// --sam: darwin.<thread>.sam beside darwin.<thread>.out
static std::string sam_name(int cpu_id)
{
    const std::string out = out_name(cpu_id);
    return out.substr(0, out.size() - 3) + "sam";
}

// darwin.cpp:314-398: the -DGPU build recodes every base in place before GACT_Batch; anything else stays
static void recode_in_place(std::vector<std::string> &seqs)
{
    for (std::string &r : seqs)
        for (char &c : r)
            switch (c) { case 'A': c = 0; break; case 'C': c = 1; break; case 'T': c = 2; break; case 'G': c = 3; break; default: break; }
}

static void feeder(int cpu_id, const std::vector<Cand> *all, size_t lo, size_t hi, GPU_storage s)
{
    std::ofstream fout(out_name(cpu_id));
    const Tick t0 = now();
    std::vector<GACT_call> calls_for, calls_rev;
    for (size_t k = lo; k < hi; k++) {
        const Cand &c = (*all)[k];
        GACT_call g;                                  // darwin.cpp:227-238
        g.ref_id = c.ref_id; g.query_id = c.query_id;
        g.ref_pos = c.ref_pos; g.query_pos = c.query_pos;
        g.ref_bpos = c.ref_pos; g.query_bpos = c.query_pos;
        g.score = 0; g.first_tile_score = 0; g.first = 1; g.reverse = 1;
        (c.comp ? calls_rev : calls_for).push_back(g);
    }
    GACT_Batch(calls_for, (int)calls_for.size(), false, 0, &s, match_score, mismatch_score, gap_open, gap_extend, fout);
    GACT_Batch(calls_rev, (int)calls_rev.size(), true, (int)calls_for.size(), &s, match_score, mismatch_score,
               gap_open, gap_extend, fout);
    fout.close();
    print_stage("Time GACT calling", t0, now());                 // darwin.cpp:441
}

// --sam: the placement of a feeder's reads [lo, hi) on its slot, behind its run: the one gact_hip_place_reads call, which
// darwin.<thread>.sam is written from and which --vcf takes the records to stack from.  o: the run's records as fetched,
// keep: the ones --unique left; the records chosen for the placement are the ones the feeder writes a line for
struct Placed {
    std::vector<int32_t> chosen;                  // indices into the run's records
    std::vector<gact_placement> place;            // one per chosen record
};

static void place_feeder_reads(gact_hip_engine *e, int slot, int lo, int hi, const std::vector<gact_overlap> &o,
                               const std::vector<char> &keep, int32_t nf, Placed &pd)
{
    auto check = [](int rc, const char *what) {
        if (rc != 0) { printf("\n%s failed: %s\n\n", what, gact_hip_last_error()); exit(-1); }
    };
    const int32_t n = (int32_t)o.size();
    // 1 the summaries of the chosen records: the placement's intervals begin where the alignments do
    std::vector<int32_t> &chosen = pd.chosen;
    for (int32_t k = 0; k < n; k++)
        if (o[(size_t)k].emitted && keep[(size_t)k]) chosen.push_back(k);
    const int32_t n_chosen = (int32_t)chosen.size();
    std::vector<gact_overlap> rec((size_t)n_chosen);
    std::vector<gact_path_summary> sums((size_t)n_chosen);
    if (n_chosen)
        check(gact_hip_candidates_summaries(e, slot, n_chosen, chosen.data(), nf, same_file, rec.data(), sums.data()),
              "gact_hip_candidates_summaries");
    // 2 the placement, over the slot's own records and the window of this feeder's reads
    std::vector<int32_t> lens((size_t)(hi - lo));
    for (int r = lo; r < hi; r++) lens[(size_t)(r - lo)] = (int32_t)reads_seqs[(size_t)r].size();
    pd.place.assign((size_t)n_chosen, gact_placement{});
    std::vector<gact_read_place> reads((size_t)(hi - lo));
    if (n_chosen)
        check(gact_hip_place_reads(e, slot, n, nullptr, n_chosen, chosen.data(), sums.data(), lo, hi - lo, lens.data(), nullptr,
                                   pd.place.data(), reads.data()), "gact_hip_place_reads");
}

// --sam: darwin.<thread>.sam from the placement of the feeder's reads
static void write_sam(gact_hip_engine *e, int slot, int cpu_id, int lo, int hi, const std::vector<gact_overlap> &o, int32_t nf,
                      const Placed &pd)
{
    auto check = [](int rc, const char *what) {
        if (rc != 0) { printf("\n%s failed: %s\n\n", what, gact_hip_last_error()); exit(-1); }
    };
    const std::vector<int32_t> &chosen = pd.chosen;
    const std::vector<gact_placement> &place = pd.place;
    const int32_t n_chosen = (int32_t)chosen.size();
    // 3 the alignments of the records to print, per read in id order, in rank order
    std::vector<int32_t> order;                   // positions in `chosen`
    for (int32_t k = 0; k < n_chosen; k++) {
        const int kind = place[(size_t)k].kind;
        if (kind == GACT_PLACE_PRIMARY || kind == GACT_PLACE_SUPPLEMENTARY ||
            (sam_mode == 2 && (kind == GACT_PLACE_SECONDARY || kind == GACT_PLACE_EXTRA)))
            order.push_back(k);
    }
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const gact_overlap &ra = o[(size_t)chosen[(size_t)a]], &rb = o[(size_t)chosen[(size_t)b]];
        return ra.query_id != rb.query_id ? ra.query_id < rb.query_id : place[(size_t)a].rank < place[(size_t)b].rank;
    });
    std::vector<int32_t> sel(order.size());
    size_t room = 1;
    for (size_t k = 0; k < order.size(); k++) {
        const gact_overlap &r = o[(size_t)chosen[(size_t)order[k]]];
        sel[k] = chosen[(size_t)order[k]];
        room += (size_t)(r.ae - r.ab) + (size_t)(r.be - r.bb);
    }
    std::vector<gact_overlap> prec(sel.size());
    std::vector<gact_path> paths(sel.size());
    std::vector<uint32_t> ops(room);
    if (!sel.empty()) {
        int64_t needed = 0;
        int rc = gact_hip_candidates_paths(e, slot, (int32_t)sel.size(), sel.data(), nf, same_file, prec.data(), paths.data(), ops.data(),
                                           (int64_t)ops.size(), &needed);
        if (rc == GACT_HIP_EINVAL && needed > (int64_t)ops.size()) {
            ops.resize((size_t)needed);
            rc = gact_hip_candidates_paths(e, slot, (int32_t)sel.size(), sel.data(), nf, same_file, prec.data(), paths.data(), ops.data(),
                                           (int64_t)ops.size(), &needed);
        }
        check(rc, "gact_hip_candidates_paths");
    }
    // 4 the file: a SAM file of its own
    std::ofstream fsam(sam_name(cpu_id));
    fsam << "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t r = 0; r < reference_seqs.size(); r++)
        fsam << "@SQ\tSN:" << reference_descrips[r][0] << "\tLN:" << reference_seqs[r].size() << "\n";
    fsam << "@PG\tID:darwin_hip\tPN:darwin_hip\n";
    std::vector<char> line;
    auto put = [&](int64_t len) {                 // false: the line needs more room than it had
        if (len < 0) { printf("\ngact_hip_format_sam failed: %s\n\n", gact_hip_last_error()); exit(-1); }
        if (len >= (int64_t)line.size()) { line.resize((size_t)len + 1); return false; }
        fsam.write(line.data(), (std::streamsize)len);
        return true;
    };
    size_t next = 0;
    for (int r = lo; r < hi; r++) {
        const std::string &seq = reads_seqs[(size_t)r];
        const char *name = reads_descrips[(size_t)r][0].c_str();
        line.resize(std::max(line.size(), 2 * seq.size() + 1024));
        const size_t first = next;
        for (; next < order.size() && o[(size_t)sel[next]].query_id == r; next++) {
            const gact_overlap &rr = o[(size_t)sel[next]];
            const gact_path &p = paths[next];
            for (int attempt = 0; attempt < 2; attempt++)
                if (put(gact_hip_format_sam(&rr, ops.data() + p.op_offset, p.n_ops, &place[(size_t)order[next]], name,
                                            (const uint8_t *)seq.data(), (int64_t)seq.size(), reference_descrips[(size_t)rr.ref_id][0].c_str(),
                                            line.data(), (int64_t)line.size())))
                    break;
        }
        if (next == first)
            for (int attempt = 0; attempt < 2; attempt++)
                if (put(gact_hip_format_sam_unmapped(name, (const uint8_t *)seq.data(), (int64_t)seq.size(), line.data(), (int64_t)line.size())))
                    break;
    }
}

// --device-dsoft: reads [lo, hi) are filtered and extended on the device, slot s.slot
static void device_feeder(int cpu_id, int lo, int hi, GPU_storage s, std::vector<Cand> *dump)
{
    gact_hip_engine *e = (gact_hip_engine *)s.engine;
    std::ofstream fout(out_name(cpu_id));
    int32_t nf = 0, nr = 0;
    float ms = 0;
    auto check = [](int rc, const char *what) {
        if (rc != 0) { printf("\n%s failed: %s\n\n", what, gact_hip_last_error()); exit(-1); }
    };
    const Tick t0 = now();
    check(gact_hip_dsoft_query(e, s.slot, lo, hi - lo, &nf, &nr, &ms), "gact_hip_dsoft_query");
    const Tick t1 = now();
    print_stage("Time finding seeds", t0, t1);                   // darwin.cpp:300
    const int32_t n = nf + nr;
    if (dump) {
        std::vector<gact_candidate> c((size_t)n);
        check(gact_hip_candidates_download(e, s.slot, n, c.data()), "gact_hip_candidates_download");
        for (int32_t k = 0; k < n; k++) dump->push_back(Cand{c[k].ref_id, c[k].query_id, c[k].ref_pos, c[k].query_pos, k >= nf});
        return;
    }
    std::vector<gact_overlap> o((size_t)n);
    check(gact_hip_candidates_run_mixed(e, s.slot, 0, n, nf, same_file), "gact_hip_candidates_run_mixed");
    check(gact_hip_candidates_fetch(e, s.slot, n, o.data()), "gact_hip_candidates_fetch");
    // --unique: which of the records to keep, chosen on the device among the slot's records (ascending, emitted ones only)
    std::vector<char> keep((size_t)n, 1);
    if (unique_mode >= 0) {
        std::vector<int32_t> kept((size_t)n);
        int32_t n_kept = 0;
        check(gact_hip_select_overlaps(e, s.slot, n, nullptr, unique_mode, kept.data(), n, &n_kept), "gact_hip_select_overlaps");
        std::fill(keep.begin(), keep.end(), 0);
        for (int32_t k = 0; k < n_kept; k++) keep[(size_t)kept[(size_t)k]] = 1;
    }
    // --min-identity: the summaries of the emitted (--unique: selected) records and one gact_hip_filter_overlaps call over the
    // slot's own records; what it keeps goes into `keep`, and the kept records' summaries serve --paf
    std::vector<gact_path_summary> kept_sums;
    if (want_filter) {
        std::vector<int32_t> chosen;
        for (int32_t k = 0; k < n; k++)
            if (o[(size_t)k].emitted && keep[(size_t)k]) chosen.push_back(k);
        const int32_t n_chosen = (int32_t)chosen.size();
        std::vector<gact_overlap> rec((size_t)n_chosen);
        std::vector<gact_path_summary> all_sums((size_t)n_chosen);
        std::vector<int32_t> kept_at((size_t)n_chosen), kept_sel((size_t)n_chosen);
        int32_t n_kept = 0;
        gact_filter_stats fs{};
        if (n_chosen) {
            check(gact_hip_candidates_summaries(e, s.slot, n_chosen, chosen.data(), nf, same_file, rec.data(), all_sums.data()),
                  "gact_hip_candidates_summaries");
            // with a D the table covers this feeder's reads [lo, hi), whose records are all on this slot: the rule is complete
            check(gact_hip_filter_overlaps(e, s.slot, n, nullptr, n_chosen, chosen.data(), all_sums.data(),
                                           filter_relative ? GACT_COVER_QUERY : GACT_COVER_BOTH, filter_relative ? lo : 0,
                                           filter_relative ? hi - lo : 0, &filter_params, nullptr, kept_at.data(), kept_sel.data(),
                                           n_chosen, &n_kept, nullptr), "gact_hip_filter_overlaps");
            check(gact_hip_last_filter_stats(e, s.slot, &fs), "gact_hip_last_filter_stats");
        }
        std::fill(keep.begin(), keep.end(), 0);
        kept_sums.resize((size_t)n_kept);
        for (int32_t k = 0; k < n_kept; k++) {
            keep[(size_t)kept_sel[(size_t)k]] = 1;
            kept_sums[(size_t)k] = all_sums[(size_t)kept_at[(size_t)k]];
        }
        printf("Filter (thread %d): kept %lld of %lld counted records; dropped: %lld empty, %lld identity, %lld span, %lld relative\n",
               cpu_id, (long long)fs.kept, (long long)fs.counted, (long long)fs.empty, (long long)fs.identity, (long long)fs.span,
               (long long)fs.relative);
    }
    // --cigar: the alignments of the emitted (--unique: selected) candidates, a second pass on the device (gact_hip_candidates_paths)
    std::vector<int32_t> sel;
    std::vector<gact_path> paths;
    std::vector<uint32_t> ops;
    // room for every op at once: an alignment has no more ops than columns, and no more columns than the bases of its
    // record's two spans (its ops end at (ae, be) and start at (ab, bb) or inside those spans, include/gact_hip.h)
    size_t room = 1;
    if (want_cigar || want_paf || pileup_depth)
        for (int32_t k = 0; k < n; k++)
            if (o[(size_t)k].emitted && keep[(size_t)k]) {
                sel.push_back(k);
                room += (size_t)(o[(size_t)k].ae - o[(size_t)k].ab) + (size_t)(o[(size_t)k].be - o[(size_t)k].bb);
            }
    if (want_cigar) {
        std::vector<gact_overlap> rec(sel.size());
        paths.resize(sel.size());
        ops.resize(room);
        int64_t needed = 0;
        int rc = sel.empty() ? 0 : gact_hip_candidates_paths(e, s.slot, (int32_t)sel.size(), sel.data(), nf, same_file, rec.data(),
                                                             paths.data(), ops.data(), (int64_t)ops.size(), &needed);
        if (rc == GACT_HIP_EINVAL && needed > (int64_t)ops.size()) {
            ops.resize((size_t)needed);
            rc = gact_hip_candidates_paths(e, s.slot, (int32_t)sel.size(), sel.data(), nf, same_file, rec.data(), paths.data(),
                                           ops.data(), (int64_t)ops.size(), &needed);
        }
        check(rc, "gact_hip_candidates_paths");
    }
    // --paf: their summaries, one more pass on the device that keeps no alignment (gact_hip_candidates_summaries)
    std::vector<gact_path_summary> sums(sel.size());
    std::ofstream fpaf;
    if (want_paf) {
        std::vector<gact_overlap> rec(sel.size());
        if (want_filter) sums = kept_sums;                                    // (of the same records in the same order: no second call)
        else
            check(gact_hip_candidates_summaries(e, s.slot, (int32_t)sel.size(), sel.data(), nf, same_file, rec.data(), sums.data()),
                  "gact_hip_candidates_summaries");
        fpaf.open(paf_name(cpu_id));
    }
    // --sam: where every read of this feeder goes (gact_hip_place_reads), for its SAM file and for --vcf
    Placed placed;
    if (sam_mode) place_feeder_reads(e, s.slot, lo, hi, o, keep, nf, placed);
    // --pileup: the same records' alignments onto their target sequences, counted on the device (gact_hip_pileup_add).  With
    // --vcf and --sam only the records the placement made primary or supplementary: a read that maps onto several copies of a
    // repeat votes once
    if (pileup_depth) {
        std::vector<int32_t> parents;
        if (want_vcf && sam_mode)
            for (size_t k = 0; k < placed.chosen.size(); k++)
                if (placed.place[k].kind == GACT_PLACE_PRIMARY || placed.place[k].kind == GACT_PLACE_SUPPLEMENTARY)
                    parents.push_back(placed.chosen[k]);
        const std::vector<int32_t> &stacked = want_vcf && sam_mode ? parents : sel;
        check(gact_hip_pileup_add(e, s.slot, (int32_t)stacked.size(), stacked.data(), nf, same_file), "gact_hip_pileup_add");
    }
    char line[1024];
    size_t next = 0;                              // (the emitted records in order: paths[next], sums[next] are this one's)
    for (int32_t at = 0; at < n; at++) {
        const gact_overlap &r = o[(size_t)at];
        if (!r.emitted || !keep[(size_t)at]) continue;
        if (coverage_depth || want_gfa) {
            cover_records[(size_t)cpu_id].push_back(r);
            if (want_paf) cover_sums[(size_t)cpu_id].push_back(sums[next]);
        }
        const int len = gact_hip_format_overlap(&r, reference_descrips[r.ref_id][0].c_str(),
                                                reads_descrips[r.query_id][0].c_str(), line, sizeof line);
        std::string cigar;
        if (want_cigar) {
            static const char kOp[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
            const gact_path &p = paths[next];
            for (int32_t k = 0; k < p.n_ops; k++) {
                const uint32_t w = ops[(size_t)(p.op_offset + k)];
                cigar += std::to_string(w >> 4);
                cigar += kOp[w & 15];
            }
            std::string text(line, (size_t)(len - 1));            // (without its newline)
            text += ", cigar: ";
            text += cigar;
            text += '\n';
            fout.write(text.data(), (std::streamsize)text.size());
        } else {
            fout.write(line, len);
        }
        if (want_paf) {
            const gact_path_summary &sm = sums[next];
            if (sm.n_eq + sm.n_x + sm.ins_bases + sm.del_bases > 0) {        // (a record without an alignment has no PAF line)
                char paf[2048];
                const int plen = gact_hip_format_paf(&r, &sm, reads_descrips[r.query_id][0].c_str(),
                                                     (int64_t)reads_seqs[r.query_id].size(), reference_descrips[r.ref_id][0].c_str(),
                                                     (int64_t)reference_seqs[r.ref_id].size(), paf, sizeof paf);
                if (plen <= 0 || plen >= (int)sizeof paf) { printf("\ngact_hip_format_paf failed: %s\n\n", gact_hip_last_error()); exit(-1); }
                std::string text(paf, (size_t)(plen - 1));
                if (want_cigar) { text += "\tcg:Z:"; text += cigar; }
                text += '\n';
                fpaf.write(text.data(), (std::streamsize)text.size());
            }
        }
        next++;
    }
    if (sam_mode) write_sam(e, s.slot, cpu_id, lo, hi, o, nf, placed);
    print_stage("Time GACT calling", t1, now());                 // darwin.cpp:441
}

// --coverage: one call over the records all feeders kept, on slot 0, then darwin.cover.tsv; the spans go to `spans` for --gfa
static int write_coverage(gact_hip_engine *e, std::vector<int32_t> *spans)
{
    std::vector<gact_overlap> rec;
    std::vector<gact_path_summary> sums;
    for (const auto &v : cover_records) rec.insert(rec.end(), v.begin(), v.end());
    for (const auto &v : cover_sums) sums.insert(sums.end(), v.begin(), v.end());
    const std::vector<std::string> &seqs = same_file ? reads_seqs : reference_seqs;
    const std::vector<std::vector<std::string> > &names = same_file ? reads_descrips : reference_descrips;
    std::vector<int32_t> lens(seqs.size());
    for (size_t i = 0; i < seqs.size(); i++) lens[i] = (int32_t)seqs[i].size();
    std::vector<gact_read_cover> cover(seqs.size());
    const int rc = gact_hip_read_coverage(e, 0, (int32_t)rec.size(), rec.data(), 0, nullptr, want_paf ? sums.data() : nullptr,
                                          same_file ? GACT_COVER_BOTH : GACT_COVER_REF, coverage_depth, (int32_t)lens.size(),
                                          lens.data(), cover.data(), nullptr);
    if (rc != 0) { printf("\ngact_hip_read_coverage failed: %s\n\n", gact_hip_last_error()); return 1; }
    if (spans)
        for (const gact_read_cover &c : cover) { spans->push_back(c.span_begin); spans->push_back(c.span_end); }
    FILE *f = fopen("darwin.cover.tsv", "w");
    if (!f) { fprintf(stderr, "--coverage: cannot write darwin.cover.tsv\n"); return 1; }
    for (size_t i = 0; i < cover.size(); i++) {
        const gact_read_cover &c = cover[i];
        fprintf(f, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\n", names[i][0].c_str(), lens[i], c.n_intervals, c.max_depth, c.covered,
                c.well_covered, c.span_begin, c.span_end, lens[i] ? (double)c.depth_sum / lens[i] : 0.0);
    }
    fclose(f);
    return 0;
}

// --unitigs: one call over what the graph call of --gfa returned, on slot 0, then darwin.utg.gfa
static int write_unitigs(gact_hip_engine *e, const std::vector<int32_t> &lens, const std::vector<int32_t> &clip,
                         const std::vector<gact_graph_read> &reads, const std::vector<gact_graph_arc> &arcs, int64_t n_arcs)
{
    const size_t n = lens.size();
    int64_t room = 0, seq_len = 0;
    for (size_t i = 0; i < n; i++) room += clip.empty() ? lens[i] : clip[2 * i + 1] - clip[2 * i];      // (every read is placed once at most)
    std::vector<gact_unitig> utg(n);
    std::vector<gact_unitig_entry> layout(n);
    std::vector<gact_unitig_place> places(n);
    std::vector<uint8_t> seq((size_t)room + 1);
    int32_t n_utg = 0;
    const gact_unitig_params params = {unitig_tips};
    const int rc = gact_hip_unitigs(e, 0, (int32_t)n, lens.data(), clip.empty() ? nullptr : clip.data(), reads.data(), n_arcs,
                                    arcs.data(), &params, utg.data(), &n_utg, layout.data(), places.data(), seq.data(), room, &seq_len);
    if (rc != 0) { printf("\ngact_hip_unitigs failed: %s\n\n", gact_hip_last_error()); return 1; }
    FILE *f = fopen("darwin.utg.gfa", "w");
    if (!f) { fprintf(stderr, "--unitigs: cannot write darwin.utg.gfa\n"); return 1; }
    fprintf(f, "H\tVN:Z:1.0\n");
    auto name = [&](int32_t j) {
        char buf[32];
        snprintf(buf, sizeof buf, "utg%06d%c", j + 1, utg[(size_t)j].circular ? 'c' : 'l');
        return std::string(buf);
    };
    for (int32_t j = 0; j < n_utg; j++) {
        const gact_unitig &u = utg[(size_t)j];
        fprintf(f, "S\t%s\t", name(j).c_str());
        fwrite(seq.data() + u.seq_at, 1, (size_t)u.length, f);
        fprintf(f, "\tLN:i:%lld\n", (long long)u.length);
        for (int32_t r = 0; r < u.n_reads; r++) {
            const gact_unitig_entry &en = layout[(size_t)(u.layout_at + r)];
            const size_t i = (size_t)(en.vertex >> 1);
            fprintf(f, "a\t%s\t%lld\t%s:%d-%d\t%c\t%d\n", name(j).c_str(), (long long)en.start, reads_descrips[i][0].c_str(),
                    clip.empty() ? 0 : clip[2 * i], clip.empty() ? lens[i] : clip[2 * i + 1], en.vertex & 1 ? '-' : '+', en.take);
        }
    }
    for (int64_t k = 0; k < n_arcs; k++) {
        const gact_graph_arc &a = arcs[(size_t)k];
        const gact_unitig_place &pu = places[(size_t)(a.u >> 1)], &pv = places[(size_t)(a.v >> 1)];
        if (a.flags || pu.state != GACT_UNITIG_PLACED || pv.state != GACT_UNITIG_PLACED) continue;       // (not an arc of E1)
        const bool fu = pu.orient == (a.u & 1), fv = pv.orient == (a.v & 1);
        // a join inside a unitig: the two vertices are neighbours in it, in the order the arc's direction gives
        if (pu.unitig == pv.unitig && fu == fv && pv.rank == pu.rank + (fu ? 1 : -1)) continue;
        fprintf(f, "L\t%s\t%c\t%s\t%c\t%dM\n", name(pu.unitig).c_str(), fu ? '+' : '-', name(pv.unitig).c_str(), fv ? '+' : '-',
                std::min(a.ov_u, a.ov_v));
    }
    fclose(f);
    return 0;
}

// --bubbles: behind the graph call, on slot 0: one unitig call without bases to learn the tips, then gact_hip_pop_bubbles with
// those tips as skip, then darwin.bubbles.tsv; arc_flags goes into the flags of `arcs`, which the unitig call of --unitigs takes
static int pop_bubbles(gact_hip_engine *e, const std::vector<int32_t> &lens, const std::vector<int32_t> &clip,
                       const std::vector<gact_graph_read> &reads, std::vector<gact_graph_arc> &arcs, int64_t n_arcs)
{
    const size_t n = lens.size();
    const int32_t *clip_p = clip.empty() ? nullptr : clip.data();
    std::vector<gact_unitig> utg(n);
    std::vector<gact_unitig_entry> layout(n);
    std::vector<gact_unitig_place> places(n);
    int32_t n_utg = 0;
    const gact_unitig_params tips = {unitig_tips};
    int rc = gact_hip_unitigs(e, 0, (int32_t)n, lens.data(), clip_p, reads.data(), n_arcs, arcs.data(), &tips, utg.data(), &n_utg,
                              layout.data(), places.data(), nullptr, 0, nullptr);
    if (rc != 0) { printf("\ngact_hip_unitigs failed: %s\n\n", gact_hip_last_error()); return 1; }
    std::vector<uint8_t> skip(n);
    for (size_t i = 0; i < n; i++) skip[i] = places[i].state == GACT_UNITIG_TIP;
    const gact_bubble_params params = {bubble_dist, GACT_BUBBLE_MAX_VERTICES};
    std::vector<gact_bubble> bubbles(2 * n + 1);                     // (a bubble per vertex at most)
    std::vector<int32_t> read_bubble(n), arc_flags((size_t)n_arcs + 1);
    int64_t n_bubbles = 0;
    rc = gact_hip_pop_bubbles(e, 0, (int32_t)n, lens.data(), clip_p, reads.data(), n_arcs, arcs.data(), skip.data(), &params,
                              bubbles.data(), (int64_t)bubbles.size(), &n_bubbles, read_bubble.data(), arc_flags.data());
    if (rc != 0) { printf("\ngact_hip_pop_bubbles failed: %s\n\n", gact_hip_last_error()); return 1; }
    FILE *f = fopen("darwin.bubbles.tsv", "w");
    if (!f) { fprintf(stderr, "--bubbles: cannot write darwin.bubbles.tsv\n"); return 1; }
    for (int64_t j = 0; j < n_bubbles; j++) {
        const gact_bubble &b = bubbles[(size_t)j];
        fprintf(f, "%d\t%d\t%d\t%d\t%d\t%d\t%lld\n", b.source, b.sink, b.state, b.n_vertices, b.n_path, b.n_removed, (long long)b.path_len);
    }
    fclose(f);
    for (int64_t k = 0; k < n_arcs; k++) arcs[(size_t)k].flags = arc_flags[(size_t)k];
    return 0;
}

// --clean: behind the graph call, on slot 0: the cleaning rounds, then darwin.clean.tsv; arc_flags goes into the flags of `arcs`,
// which the unitig call of --unitigs takes
static int clean_graph(gact_hip_engine *e, const std::vector<int32_t> &lens, const std::vector<int32_t> &clip,
                       const std::vector<gact_graph_read> &reads, std::vector<gact_graph_arc> &arcs, int64_t n_arcs)
{
    const size_t n = lens.size();
    const gact_clean_params params = {unitig_tips, bubble_dist ? bubble_dist : GACT_BUBBLE_DEFAULT_MAX_DIST, GACT_BUBBLE_MAX_VERTICES,
                                      clean_lo, clean_hi, clean_n, 4};
    std::vector<gact_clean_step> steps((size_t)(params.n_ratios + 1) * (2 * params.max_passes + 1));   // (always suffices)
    std::vector<gact_clean_read> state(n + 1);
    std::vector<int32_t> arc_flags((size_t)n_arcs + 1);
    int64_t n_steps = 0;
    const int rc = gact_hip_clean_graph(e, 0, (int32_t)n, lens.data(), clip.empty() ? nullptr : clip.data(), reads.data(), n_arcs,
                                        arcs.data(), &params, arc_flags.data(), state.data(), steps.data(), (int64_t)steps.size(), &n_steps);
    if (rc != 0) { printf("\ngact_hip_clean_graph failed: %s\n\n", gact_hip_last_error()); return 1; }
    FILE *f = fopen("darwin.clean.tsv", "w");
    if (!f) { fprintf(stderr, "--clean: cannot write darwin.clean.tsv\n"); return 1; }
    static const char *const kinds[3] = {"tips", "bubbles", "prune"};
    for (int64_t j = 0; j < n_steps; j++) {
        const gact_clean_step &s = steps[(size_t)j];
        fprintf(f, "%lld\t%s\t%d\t%d\t%d\t%lld\t%lld\n", (long long)j, kinds[s.kind], s.param, s.reads_removed, s.examined,
                (long long)s.arcs_removed, (long long)s.arcs_left);
    }
    fclose(f);
    for (int64_t k = 0; k < n_arcs; k++) arcs[(size_t)k].flags = arc_flags[(size_t)k];
    return 0;
}

// --gfa: one call over the records all feeders kept, on slot 0, then darwin.gfa.  clip: the spans of --coverage, or empty
static int write_gfa(gact_hip_engine *e, const std::vector<int32_t> &clip)
{
    std::vector<gact_overlap> rec;
    std::vector<gact_path_summary> sums;
    for (const auto &v : cover_records) rec.insert(rec.end(), v.begin(), v.end());
    for (const auto &v : cover_sums) sums.insert(sums.end(), v.begin(), v.end());
    std::vector<int32_t> lens(reads_seqs.size());
    for (size_t i = 0; i < reads_seqs.size(); i++) lens[i] = (int32_t)reads_seqs[i].size();
    std::vector<gact_graph_read> reads(lens.size());
    std::vector<gact_graph_arc> arcs(2 * rec.size() + 1);            // (twice the chosen count always suffices)
    int64_t n_arcs = 0;
    const int rc = gact_hip_overlap_graph(e, 0, (int32_t)rec.size(), rec.data(), 0, nullptr, want_paf ? sums.data() : nullptr,
                                          (int32_t)lens.size(), lens.data(), clip.empty() ? nullptr : clip.data(), nullptr,
                                          reads.data(), nullptr, arcs.data(), (int64_t)arcs.size(), &n_arcs);
    if (rc != 0) { printf("\ngact_hip_overlap_graph failed: %s\n\n", gact_hip_last_error()); return 1; }
    FILE *f = fopen("darwin.gfa", "w");
    if (!f) { fprintf(stderr, "--gfa: cannot write darwin.gfa\n"); return 1; }
    fprintf(f, "H\tVN:Z:1.0\n");
    for (size_t i = 0; i < reads.size(); i++) {
        const int32_t b = clip.empty() ? 0 : clip[2 * i], end = clip.empty() ? lens[i] : clip[2 * i + 1];
        if (reads[i].contained_by >= 0 || end <= b) continue;
        fprintf(f, "S\t%s\t%.*s\tLN:i:%d\n", reads_descrips[i][0].c_str(), (int)(end - b), reads_seqs[i].c_str() + b, (int)(end - b));
    }
    for (int64_t k = 0; k < n_arcs; k++) {
        const gact_graph_arc &a = arcs[(size_t)k];
        if (a.flags) continue;
        fprintf(f, "L\t%s\t%c\t%s\t%c\t%dM\tL1:i:%d\n", reads_descrips[(size_t)(a.u >> 1)][0].c_str(), a.u & 1 ? '-' : '+',
                reads_descrips[(size_t)(a.v >> 1)][0].c_str(), a.v & 1 ? '-' : '+', std::min(a.ov_u, a.ov_v), a.len);
    }
    fclose(f);
    // (darwin.gfa is written: the arcs may change)
    if (clean_lo >= 0 ? clean_graph(e, lens, clip, reads, arcs, n_arcs) : bubble_dist && pop_bubbles(e, lens, clip, reads, arcs, n_arcs)) return 1;
    return unitig_tips >= 0 ? write_unitigs(e, lens, clip, reads, arcs, n_arcs) : 0;
}

// --pileup: the consensus of every reference sequence from the counts the feeders' adds left, then darwin.cons.fa
static int write_consensus(gact_hip_engine *e)
{
    size_t positions = 0;
    for (const std::string &r : reference_seqs) positions += r.size();
    std::vector<uint8_t> cons(positions);
    std::vector<gact_read_pileup> table(reference_seqs.size());
    if (gact_hip_pileup_finish(e, pileup_depth, nullptr, cons.data(), table.data()) != 0) {
        printf("\ngact_hip_pileup_finish failed: %s\n\n", gact_hip_last_error());
        return 1;
    }
    // --ins-slots: the corrected reads come spelled from the device, back to back
    std::vector<gact_read_corrected> corrected;
    std::vector<int64_t> read_at;
    std::vector<uint8_t> spelled;
    if (pileup_ins_slots) {
        corrected.resize(reference_seqs.size());
        read_at.resize(reference_seqs.size() + 1);
        spelled.resize(positions * (size_t)(pileup_ins_slots + 1));         // (always suffices)
        int64_t n_spelled = 0;
        if (gact_hip_pileup_corrected(e, pileup_depth, nullptr, corrected.data(), read_at.data(), spelled.data(), (int64_t)spelled.size(),
                                      &n_spelled) != 0) {
            printf("\ngact_hip_pileup_corrected failed: %s\n\n", gact_hip_last_error());
            return 1;
        }
    }
    FILE *f = fopen("darwin.cons.fa", "w");
    if (!f) { fprintf(stderr, "--pileup: cannot write darwin.cons.fa\n"); return 1; }
    size_t at = 0;
    std::string seq;
    for (size_t i = 0; i < reference_seqs.size(); i++) {
        const gact_read_pileup &t = table[i];
        if (pileup_ins_slots) {
            fprintf(f, ">%s called=%d changed=%d deleted=%d ins_flagged=%d inserted=%d\n", reference_descrips[i][0].c_str(), t.called,
                    t.changed, t.deleted, t.ins_flagged, corrected[i].inserted);
            fwrite(spelled.data() + read_at[i], 1, (size_t)(read_at[i + 1] - read_at[i]), f);
            fputc('\n', f);
            continue;
        }
        fprintf(f, ">%s called=%d changed=%d deleted=%d ins_flagged=%d\n", reference_descrips[i][0].c_str(), t.called, t.changed,
                t.deleted, t.ins_flagged);
        seq.clear();
        for (size_t k = 0; k < reference_seqs[i].size(); k++)
            if (cons[at + k] != '-') seq += (char)cons[at + k];
        at += reference_seqs[i].size();
        fprintf(f, "%s\n", seq.c_str());
    }
    fclose(f);
    return 0;
}

// --vcf: the variants of every reference sequence from the same counts, one gact_hip_pileup_variants call, then darwin.vcf
static int write_variants(gact_hip_engine *e)
{
    const gact_variant_params params = {pileup_depth, vcf_min_alt, vcf_min_permille, vcf_hom_permille};
    std::vector<gact_variant> v(1024);
    int64_t n = 0;
    int rc = gact_hip_pileup_variants(e, &params, v.data(), (int64_t)v.size(), &n, nullptr);
    if (rc == GACT_HIP_EINVAL && n > (int64_t)v.size()) {
        v.resize((size_t)n);
        rc = gact_hip_pileup_variants(e, &params, v.data(), (int64_t)v.size(), &n, nullptr);
    }
    if (rc != 0) { printf("\ngact_hip_pileup_variants failed: %s\n\n", gact_hip_last_error()); return 1; }
    FILE *f = fopen("darwin.vcf", "w");
    if (!f) { fprintf(stderr, "--vcf: cannot write darwin.vcf\n"); return 1; }
    fprintf(f, "##fileformat=VCFv4.2\n");
    for (size_t i = 0; i < reference_seqs.size(); i++)
        fprintf(f, "##contig=<ID=%s,length=%zu>\n", reference_descrips[i][0].c_str(), reference_seqs[i].size());
    fprintf(f, "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Alignments that span the position\">\n"
               "##INFO=<ID=AD,Number=1,Type=Integer,Description=\"Alignments that support the alternate allele\">\n"
               "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype by the thresholds min_alt=%d min_permille=%d hom_permille=%d at depth >= %d\">\n"
               "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tdarwin\n",
            vcf_min_alt, vcf_min_permille, vcf_hom_permille, pileup_depth);
    std::vector<char> line(4096);
    for (int64_t k = 0; k < n; k++) {
        const gact_variant &r = v[(size_t)k];
        if (r.seq < 0 || (size_t)r.seq >= reference_seqs.size()) { fprintf(stderr, "--vcf: record %lld names sequence %d\n", (long long)k, r.seq); fclose(f); return 1; }
        const std::string &seq = reference_seqs[(size_t)r.seq];
        for (int attempt = 0; attempt < 2; attempt++) {
            const int len = gact_hip_format_vcf(&r, reference_descrips[(size_t)r.seq][0].c_str(), (const uint8_t *)seq.data(),
                                                (int64_t)seq.size(), line.data(), line.size());
            if (len < 0) { printf("\ngact_hip_format_vcf failed: %s\n\n", gact_hip_last_error()); fclose(f); return 1; }
            if ((size_t)len < line.size()) { fwrite(line.data(), 1, (size_t)len, f); break; }
            line.resize((size_t)len + 1);
        }
    }
    fclose(f);
    return 0;
}

// --rccl-gather IDFILE (with --shard R/W): this rank's share as ONE run on the engine (no feeder threads: a run is fastest
// with all of its candidates in one launch), then the job's one collective -- every rank's records to rank 0 over RCCL,
// out of the engines' device arrays (gact_hip_comm_gather_lines) -- and rank 0 writes darwin.gathered.out: the lines of
// rank 0, then rank 1's, ..., each rank's forward-strand lines first.  `cat darwin.*.out | sort | uniq` of the file-based
// form and `sort | uniq` of this file are the same lines.
static int gathered_run(const std::vector<std::vector<Cand> > &per_thread, const std::string &id_path)
{
    auto check = [](int rc, const char *what) {
        if (rc != 0) { printf("\n%s failed: %s\n\n", what, gact_hip_last_error()); exit(-1); }
    };
    std::vector<gact_candidate> cands;
    for (int comp = 0; comp < 2; comp++)
        for (const auto &v : per_thread)
            for (const Cand &c : v)
                if ((c.comp != 0) == (comp != 0)) cands.push_back(gact_candidate{c.ref_id, c.query_id, c.ref_pos, c.query_pos});
    int32_t nf = 0;
    for (const auto &v : per_thread)
        for (const Cand &c : v) nf += c.comp ? 0 : 1;
    const int32_t n = (int32_t)cands.size();
    std::vector<GPU_storage> s;
    GPU_init(tile_size, tile_overlap, gap_open, gap_extend, match_score, mismatch_score, tile_size - tile_overlap, &s, 1);
    gact_hip_engine *e = (gact_hip_engine *)s[0].engine;
    gact_hip_comm *comm = nullptr;
    check(gact_hip_comm_create(e, shard_rank, shard_world, id_path.c_str(), 0, &comm), "gact_hip_comm_create");
    const Tick t0 = now();
    check(gact_hip_candidates_upload(e, 0, n, cands.data()), "gact_hip_candidates_upload");
    check(gact_hip_candidates_run_mixed(e, 0, 0, n, nf, same_file), "gact_hip_candidates_run_mixed");
    const Tick t1 = now();
    std::vector<int64_t> counts((size_t)shard_world, 0);
    // (rank 0 cannot know the total before the call: room for every rank's share at its largest -- the deal is round-robin)
    std::vector<gact_line> lines(shard_rank == 0 ? ((size_t)n + 1) * (size_t)shard_world : 0);
    check(gact_hip_comm_gather_lines(comm, 0, n, counts.data(), shard_rank == 0 ? lines.data() : nullptr, (int64_t)lines.size()),
          "gact_hip_comm_gather_lines");
    const Tick t2 = now();
    print_stage("Time GACT calling", t0, t1);                                   // darwin.cpp:441 (launch; the wait is in the gather)
    print_stage("Time gathering records (RCCL)", t1, t2);
    if (shard_rank == 0) {
        int64_t total = 0;
        printf("gathered records per rank:");
        for (int r = 0; r < shard_world; r++) { printf(" %lld", (long long)counts[(size_t)r]); total += counts[(size_t)r]; }
        printf("\n");
        std::ofstream fout("darwin.gathered.out");
        char line[1024];
        for (int64_t k = 0; k < total; k++) {
            const gact_line &l = lines[(size_t)k];
            if (!(l.comp_emitted & 2)) continue;
            gact_overlap o;
            memset(&o, 0, sizeof o);
            o.ref_id = l.ref_id; o.query_id = l.query_id; o.ab = l.ab; o.ae = l.ae; o.bb = l.bb; o.be = l.be;
            o.score = l.score; o.comp = l.comp_emitted & 1; o.emitted = 1;
            const int len = gact_hip_format_overlap(&o, reference_descrips[o.ref_id][0].c_str(), reads_descrips[o.query_id][0].c_str(),
                                                    line, sizeof line);
            fout.write(line, len);
        }
    }
    gact_hip_comm_destroy(comm);
    GPU_close(&s, 1);
    return 0;
}

static void upload_set(gact_hip_engine *e, int which, const std::vector<std::string> &seqs)
{
    std::vector<int64_t> offs(seqs.size() + 1, 0);
    for (size_t k = 0; k < seqs.size(); k++) offs[k + 1] = offs[k] + (int64_t)seqs[k].size();
    std::vector<uint8_t> cat((size_t)offs.back());
    for (size_t k = 0; k < seqs.size(); k++) memcpy(cat.data() + offs[k], seqs[k].data(), seqs[k].size());
    if (gact_hip_upload_seqs(e, which, cat.data(), offs.data(), (int32_t)seqs.size()) != 0) {
        printf("\nupload failed: %s\n\n", gact_hip_last_error());
        exit(-1);
    }
}

static void print_queue(const char *tag, std::queue<int> q)
{
    printf("%s", tag);
    while (!q.empty()) { printf(" %d", q.front()); q.pop(); }
    printf("\n");
}

// FILE lines:  T ref query match mismatch open ext reverse first early     -> AlignWithBT + Align_Batch_GPU
//              G ref query ref_pos query_pos tile overlap thr match mismatch open ext comp -> GACT
static int selftest(const char *path)
{
    std::ifstream in(path);
    std::string kind;
    std::vector<GPU_storage> s;
    bool inited = false;
    int n = 0;
    while (in >> kind) {
        if (kind == "T") {
            std::string r, q; int m, x, o, e, rev, first, early;
            in >> r >> q >> m >> x >> o >> e >> rev >> first >> early;
            print_queue("AlignWithBT", AlignWithBT((char *)r.c_str(), (long long)r.size(), (char *)q.c_str(),
                                                   (long long)q.size(), m, x, o, e, (int)q.size(), (int)r.size(),
                                                   rev != 0, first != 0, early));
            if (m == 1 && x == -1 && o == -1 && e == -1 && early == tile_size - tile_overlap &&
                (int)r.size() <= tile_size && (int)q.size() <= tile_size) {
                if (!inited) {
                    NUM_BLOCKS = 1; THREADS_PER_BLOCK = 4; BATCH_SIZE = 4;
                    GPU_init(tile_size, tile_overlap, gap_open, gap_extend, match_score, mismatch_score,
                             tile_size - tile_overlap, &s, 1);
                    inited = true;
                }
                // slot 1 of a 4-slot batch, the others idle (ref_len -1, gact.cpp:303-305)
                std::vector<std::string> rs(4), qs(4);
                std::vector<int> rl(4, -1), ql(4, 0);
                std::vector<char> rv(4, 0), fs(4, 0);
                rs[1] = r; qs[1] = q; rl[1] = (int)r.size(); ql[1] = (int)q.size();
                rv[1] = rev ? 0 : 1;      // Align_Batch_GPU's sense is the opposite of AlignWithBT's
                fs[1] = (char)first;
                int *out = Align_Batch_GPU(rs, qs, rl, ql, nullptr, gap_open, gap_extend, rl, ql, rv, fs,
                                           tile_size - tile_overlap, tile_size, &s[0], NUM_BLOCKS, THREADS_PER_BLOCK);
                const int *o1 = out + 2 * tile_size;
                printf("Align_Batch_GPU %d %d %d %d %d :", o1[0], o1[1], o1[2], o1[3], o1[4]);
                for (int k = 5; o1[k] != -1; k++) printf(" %d", o1[k]);
                printf("\n");
                free(out);
            }
        } else if (kind == "P") {
            // P ref query match mismatch open ext reverse first early ref_pos query_pos -> AlignWithBT at a position
            std::string r, q; int m, x, o, e, rev, first, early, rp, qp;
            in >> r >> q >> m >> x >> o >> e >> rev >> first >> early >> rp >> qp;
            print_queue("AlignWithBT", AlignWithBT((char *)r.c_str(), (long long)r.size(), (char *)q.c_str(),
                                                   (long long)q.size(), m, x, o, e, qp, rp, rev != 0, first != 0, early));
        } else if (kind == "B") {
            // B n match mismatch open ext early, then n lines "ref query reverse first" ("-" "-" = idle, ref_len -1)
            int nb, m, x, o, e, early;
            in >> nb >> m >> x >> o >> e >> early;
            std::vector<std::string> rs(nb), qs(nb);
            std::vector<int> rl(nb), ql(nb);
            std::vector<char> rv(nb), fs(nb);
            for (int k = 0; k < nb; k++) {
                int rev, first;
                in >> rs[k] >> qs[k] >> rev >> first;
                if (rs[k] == "-") { rs[k].clear(); qs[k].clear(); rl[k] = -1; ql[k] = 0; }     // align.cpp:40-44
                else { rl[k] = (int)rs[k].size(); ql[k] = (int)qs[k].size(); }
                rv[k] = (char)rev; fs[k] = (char)first;
            }
            std::vector<std::queue<int> > res = Align_Batch(rs, qs, rl, ql, m, x, o, e, rl, ql, rv, fs, early);
            for (int k = 0; k < nb; k++) print_queue("Align_Batch", res[k]);
        } else if (kind == "G") {
            std::string r, q; int rp, qp, t, ov, thr, m, x, o, e, comp;
            in >> r >> q >> rp >> qp >> t >> ov >> thr >> m >> x >> o >> e >> comp;
            reference_descrips.assign(1, std::vector<std::string>(1, "refname"));
            reads_descrips.assign(2, std::vector<std::string>(1, "queryname"));
            same_file = false;
            const char *tmp = "selftest_gact.out";
            { std::ofstream fout(tmp);
              GACT((char *)r.c_str(), (char *)q.c_str(), (int)r.size(), (int)q.size(), t, ov, rp, qp, thr, 0, 1,
                   comp != 0, m, x, o, e, fout); }
            std::ifstream back(tmp); std::stringstream ss; ss << back.rdbuf();
            printf("GACT %s", ss.str().empty() ? "\n" : ss.str().c_str());
            remove(tmp);
        }
        n++;
    }
    if (inited) GPU_close(&s, 1);
    return n > 0 ? 0 : 1;
}

int main(int argc, char *argv[])
{
    if (argc >= 3 && strcmp(argv[1], "--selftest") == 0) return selftest(argv[2]);
    if (argc < 4) {
        fprintf(stderr, "Usage: darwin_hip <REFERENCE>.fasta <READS>.fasta CPU_THREADS --candidates FILE "
                        "[--params params.cfg] [--device-dsoft [--cigar] [--paf] [--unique exact|pair] [--coverage K] [--pileup K [--ins-slots S] [--vcf A:P:H]] [--gfa [--unitigs K [--bubbles D] [--clean LO:HI:N]]] [--sam primary|all] [--min-identity P[:S[:D]]]]\n");
        return 1;
    }
    std::string cand_path, dump_path, cfg_path = "params.cfg", gather_id;
    bool dsoft_only = false, device_dsoft = false, recode = false, shard_given = false;
    for (int a = 4; a < argc; a++) {
        if (!strcmp(argv[a], "--candidates") && a + 1 < argc) cand_path = argv[++a];
        else if (!strcmp(argv[a], "--dump-candidates") && a + 1 < argc) dump_path = argv[++a];
        else if (!strcmp(argv[a], "--params") && a + 1 < argc) cfg_path = argv[++a];
        else if (!strcmp(argv[a], "--dsoft-only")) dsoft_only = true;
        else if (!strcmp(argv[a], "--device-dsoft")) device_dsoft = true;
        else if (!strcmp(argv[a], "--recode")) recode = true;
        else if (!strcmp(argv[a], "--cigar")) want_cigar = true;
        else if (!strcmp(argv[a], "--paf")) want_paf = true;
        else if (!strcmp(argv[a], "--unique")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            if (!strcmp(v, "exact")) unique_mode = GACT_SELECT_EXACT;
            else if (!strcmp(v, "pair")) unique_mode = GACT_SELECT_PAIR;
            else { fprintf(stderr, "--unique wants exact or pair, not '%s'\n", v); return 1; }
        }
        else if (!strcmp(argv[a], "--coverage")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (!*v || *end || k < 1 || k > 0x7fffffffL) { fprintf(stderr, "--coverage wants an integer >= 1, not '%s'\n", v); return 1; }
            coverage_depth = (int)k;
        }
        else if (!strcmp(argv[a], "--pileup")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (!*v || *end || k < 1 || k > 0x7fffffffL) { fprintf(stderr, "--pileup wants an integer >= 1, not '%s'\n", v); return 1; }
            pileup_depth = (int)k;
        }
        else if (!strcmp(argv[a], "--ins-slots")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (!*v || *end || k < 1 || k > GACT_PILEUP_MAX_INS_SLOTS) {
                fprintf(stderr, "--ins-slots wants an integer from 1 to %d, not '%s'\n", GACT_PILEUP_MAX_INS_SLOTS, v);
                return 1;
            }
            pileup_ins_slots = (int)k;
        }
        else if (!strcmp(argv[a], "--vcf")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            int alt = 0, lo = 0, hi = 0, used = 0;
            if (sscanf(v, "%d:%d:%d%n", &alt, &lo, &hi, &used) != 3 || v[used] || alt < 1 || lo < 0 || lo > hi || hi > 1000) {
                fprintf(stderr, "--vcf wants A:P:H (min_alt:min_permille:hom_permille) with A >= 1 and 0 <= P <= H <= 1000, not '%s'\n", v);
                return 1;
            }
            want_vcf = true;
            vcf_min_alt = alt; vcf_min_permille = lo; vcf_hom_permille = hi;
        }
        else if (!strcmp(argv[a], "--gfa")) want_gfa = true;
        else if (!strcmp(argv[a], "--unitigs")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (!*v || *end || k < 0 || k > 0x7fffffffL) { fprintf(stderr, "--unitigs wants an integer >= 0, not '%s'\n", v); return 1; }
            unitig_tips = (int)k;
        }
        else if (!strcmp(argv[a], "--bubbles")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (!*v || *end || k < 1 || k > (1L << 30)) { fprintf(stderr, "--bubbles wants an integer from 1 to 2^30, not '%s'\n", v); return 1; }
            bubble_dist = (int)k;
        }
        else if (!strcmp(argv[a], "--clean")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            int lo = 0, hi = 0, k = 0, used = 0;
            if (sscanf(v, "%d:%d:%d%n", &lo, &hi, &k, &used) != 3 || v[used] || lo < 0 || lo > hi || hi > 1000 || k < 0 ||
                k > GACT_CLEAN_MAX_RATIOS) {
                fprintf(stderr, "--clean wants LO:HI:N with 0 <= LO <= HI <= 1000 and 0 <= N <= %d, not '%s'\n", GACT_CLEAN_MAX_RATIOS, v);
                return 1;
            }
            clean_lo = lo; clean_hi = hi; clean_n = k;
        }
        else if (!strcmp(argv[a], "--min-identity")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            long f[3] = {0, GACT_FILTER_DEFAULT_MIN_SPAN, GACT_FILTER_DEFAULT_MAX_DROP_PERMILLE};
            int got = 0;
            bool ok = *v != 0;
            for (const char *at = v; ok && got < 3;) {
                char *end = nullptr;
                ok = *at >= '0' && *at <= '9';                               // (no sign, no blank, no empty field)
                if (ok) f[got++] = strtol(at, &end, 10);
                if (!ok || !*end) break;
                ok = *end == ':' && got < 3;
                at = end + 1;
            }
            if (!ok || f[0] > 1000 || f[1] > 0x7fffffffL || f[2] > 1000) {
                fprintf(stderr, "--min-identity wants P[:S[:D]] (min identity per mille, min span, max drop per mille under the read's "
                                "best) with integers 0 <= P <= 1000, S >= 0 and 0 <= D <= 1000, not '%s'\n", v);
                return 1;
            }
            want_filter = true;
            filter_relative = got == 3;
            filter_params.min_identity_permille = (int32_t)f[0];
            filter_params.min_span = (int32_t)f[1];
            filter_params.max_drop_permille = (int32_t)f[2];
        }
        else if (!strcmp(argv[a], "--sam")) {
            const char *v = a + 1 < argc ? argv[++a] : "";
            if (!strcmp(v, "primary")) sam_mode = 1;
            else if (!strcmp(v, "all")) sam_mode = 2;
            else { fprintf(stderr, "--sam wants primary or all, not '%s'\n", v); return 1; }
        }
        else if (!strcmp(argv[a], "--rccl-gather") && a + 1 < argc) gather_id = argv[++a];
        else if (!strcmp(argv[a], "--device") && a + 1 < argc) setenv("GACT_HIP_DEVICE", argv[++a], 1);   // read by GPU_init
        else if (!strcmp(argv[a], "--shard") && a + 1 < argc) {
            shard_given = true;
            if (sscanf(argv[++a], "%d/%d", &shard_rank, &shard_world) != 2 || shard_world < 1 || shard_rank < 0 ||
                shard_rank >= shard_world) { fprintf(stderr, "--shard wants R/W with 0 <= R < W\n"); return 1; }
        } else { fprintf(stderr, "unknown option %s\n", argv[a]); return 1; }
    }
    if (recode && device_dsoft) { fprintf(stderr, "--recode: the device filter reads ASCII sets\n"); return 1; }
    if (want_cigar && (!device_dsoft || !gather_id.empty())) {
        // the host-filter mode writes through the reference-signature GACT_Batch, which has no alignment to give; the gathered
        // output would need the CIGARs gathered too
        fprintf(stderr, "--cigar: only with --device-dsoft, and not with --rccl-gather\n");
        return 1;
    }
    if (want_paf && (!device_dsoft || !gather_id.empty())) {
        // (for the same reasons: the summaries come from the engine's own candidate arrays, and would have to be gathered)
        fprintf(stderr, "--paf: only with --device-dsoft, and not with --rccl-gather\n");
        return 1;
    }
    if (unique_mode >= 0 && (!device_dsoft || shard_world > 1)) {
        // the selection runs over the records of one engine slot: the host-filter mode writes through GACT_Batch, and the ranks of
        // a sharded job each hold part of a pair's candidates, so a selection per rank would be incomplete
        fprintf(stderr, "--unique: only with --device-dsoft, and not with --shard\n");
        return 1;
    }
    if (want_filter && (!device_dsoft || !gather_id.empty())) {
        // (as --paf: the filter reads the summaries of the engine's own candidate arrays, and the gathered lines come from the
        // device's records, which know nothing of what a feeder kept)
        fprintf(stderr, "--min-identity: only with --device-dsoft, and not with --rccl-gather\n");
        return 1;
    }
    if (coverage_depth && (!device_dsoft || shard_given)) {
        // the table is made from the records of one process's feeders: the host-filter mode keeps none (it writes through
        // GACT_Batch), and a rank of a sharded job holds part of every read's overlaps
        fprintf(stderr, "--coverage: only with --device-dsoft, and not with --shard\n");
        return 1;
    }
    if (pileup_depth && (!device_dsoft || shard_given)) {
        // the counts come from the alignments of one engine's candidate arrays, and a rank of a sharded job holds part of every
        // sequence's overlaps: combining the ranks' counts is left to the caller
        fprintf(stderr, "--pileup: only with --device-dsoft, and not with --shard\n");
        return 1;
    }
    if (pileup_ins_slots && !pileup_depth) {
        fprintf(stderr, "--ins-slots: only with --pileup\n");
        return 1;
    }
    if (want_vcf && !pileup_depth) {
        // the records are called from the counts of --pileup, whose K is their min_depth
        fprintf(stderr, "--vcf: only with --pileup\n");
        return 1;
    }
    if (want_gfa && (!device_dsoft || shard_given || strcmp(argv[1], argv[2]) != 0)) {
        // the graph is over one read set, from the records of one process's feeders: the host-filter mode keeps none, a rank of a
        // sharded job holds part of every read's overlaps, and with two files ref and query ids name different sequences
        fprintf(stderr, "--gfa: only with --device-dsoft and one input file used for both sides, and not with --shard\n");
        return 1;
    }
    if (bubble_dist && (!want_gfa || unitig_tips < 1)) {
        // the bubbles are popped between two rounds of tip cutting, the second one the unitig call's: with K == 0 no tip is cut and
        // the reads a bubble removed would come back as unitigs of one read
        fprintf(stderr, "--bubbles: only with --gfa --unitigs K and K >= 1\n");
        return 1;
    }
    if (clean_lo >= 0 && (!want_gfa || unitig_tips < 1)) {
        // (for the same reason: the rounds cut tips with K, and with K == 0 the removed reads would come back)
        fprintf(stderr, "--clean: only with --gfa --unitigs K and K >= 1\n");
        return 1;
    }
    if (unitig_tips >= 0 && !want_gfa) {
        // the unitigs are made from what the graph call of --gfa returns
        fprintf(stderr, "--unitigs: only with --gfa\n");
        return 1;
    }
    if (sam_mode && (!device_dsoft || shard_given || !gather_id.empty())) {
        // a read is placed among ALL its records, which one feeder's slot holds behind the device filter; the ranks of a sharded job
        // split the reads, and every rank's files would need a header and a name of their own: left to the caller
        fprintf(stderr, "--sam: only with --device-dsoft, and not with --shard\n");
        return 1;
    }
    std::map<std::string, double> cfg = parse_cfg(cfg_path);
    auto get = [&](const char *k, int dflt) { return cfg.count(k) ? (int)cfg[k] : dflt; };
    match_score = get("GACT_scoring/match", 1); mismatch_score = get("GACT_scoring/mismatch", -1);
    gap_open = get("GACT_scoring/gap_open", -1); gap_extend = get("GACT_scoring/gap_extend", -1);
    first_tile_score_threshold = get("GACT_first_tile/first_tile_score_threshold", 35);
    tile_size = get("GACT_extend/tile_size", 320); tile_overlap = get("GACT_extend/tile_overlap", 120);
    DsoftParams dp;
    dp.seed_size = get("DSOFT_params/seed_size", 14); dp.bin_size = (uint32_t)get("DSOFT_params/bin_size", 64);
    dp.window_size = (uint32_t)get("DSOFT_params/window_size", 4); dp.threshold = get("DSOFT_params/threshold", 21);
    dp.num_seeds = get("DSOFT_params/num_seeds", 800);
    dp.seed_occurence_multiple = (uint32_t)get("DSOFT_params/seed_occurence_multiple", 32);
    dp.max_candidates = get("DSOFT_params/max_candidates", 1000000);
    num_threads = std::stoi(argv[3]);
    if (num_threads < 1) num_threads = 1;
    const std::string ref_path(argv[1]), reads_path(argv[2]);
    same_file = (ref_path == reads_path);                         // darwin.cpp:500-502
    printf("same_file: %d\n", same_file);
    printf("Scores: match = %d, mismatch = %d, gap_open = %d, gap_extend = %d\n", match_score, mismatch_score,
           gap_open, gap_extend);

    Tick t_stage = now();
    parse_fasta(ref_path, reference_descrips, reference_seqs, reference_lengths);
    print_stage("Time elapsed (loading reference genome)", t_stage, now());      // darwin.cpp:553
    t_stage = now();
    parse_fasta(reads_path, reads_descrips, reads_seqs, reads_lengths);
    if (!device_dsoft)
        for (const std::string &r : reads_seqs) rev_reads_seqs.push_back(rev_comp(r));
    std::cout << "Number of reads: " << reads_seqs.size() << std::endl;
    print_stage("Time elapsed (loading reads)", t_stage, now());                 // darwin.cpp:574

    if (device_dsoft) {
        std::vector<GPU_storage> s;
        GPU_init(tile_size, tile_overlap, gap_open, gap_extend, match_score, mismatch_score, tile_size - tile_overlap,
                 &s, num_threads);
        gact_hip_engine *e = (gact_hip_engine *)s[0].engine;
        upload_set(e, GACT_SET_REF, reference_seqs);
        upload_set(e, GACT_SET_QUERY, reads_seqs);
        if (gact_hip_derive_revcomp(e) != 0) { std::cerr << gact_hip_last_error() << std::endl; return 1; }   // darwin.cpp:110-147
        gact_dsoft_params gp = {dp.seed_size, (int32_t)dp.bin_size, (int32_t)dp.window_size, dp.threshold, dp.num_seeds,
                                (int32_t)dp.seed_occurence_multiple, dp.max_candidates};
        gact_dsoft_info info;
        t_stage = now();
        if (gact_hip_dsoft_build(e, &gp, &info) != 0) { printf("\ndsoft_build failed: %s\n\n", gact_hip_last_error()); return 1; }
        printf("Reference length: %lld, %zu pieces; device index: %lld minimizers, %.1f ms\n", (long long)info.ref_length,
               reference_seqs.size(), (long long)info.n_minimizers, info.build_ms);
        print_stage("Time elapsed (seed position table construction)", t_stage, now());      // darwin.cpp:596
        // this rank's contiguous share of the reads, then contiguous ranges per feeder thread (darwin.cpp:619-629)
        const int all_reads = (int)reads_seqs.size();
        const int per_rank = (int)std::ceil(1.0 * all_reads / shard_world);
        const int r_lo = std::min(all_reads, shard_rank * per_rank), r_hi = std::min(all_reads, r_lo + per_rank);
        const int num_reads = r_hi - r_lo;
        const int reads_per_thread = (int)std::ceil(1.0 * num_reads / num_threads);
        std::vector<std::vector<Cand> > dumps(num_threads);
        const bool dumping = !dump_path.empty() && dsoft_only;
        cover_records.resize((size_t)num_threads);
        cover_sums.resize((size_t)num_threads);
        if (pileup_depth && !dumping && gact_hip_pileup_begin_ins(e, 0, (int32_t)reference_seqs.size(), pileup_ins_slots) != 0) {
            printf("\ngact_hip_pileup_begin_ins failed: %s\n\n", gact_hip_last_error());
            return 1;
        }
        std::vector<std::thread> threads;
        t_stage = now();
        for (int i = 0; i < num_threads; i++) {
            const int lo = r_lo + std::min(num_reads, i * reads_per_thread), hi = std::min(r_hi, lo + reads_per_thread);
            threads.push_back(std::thread(device_feeder, i, lo, hi, s[i], dumping ? &dumps[i] : nullptr));
        }
        for (auto &t : threads) t.join();
        print_stage("Time elapsed (seed table querying + aligning)", t_stage, now());         // darwin.cpp:639
        if (dumping) {
            std::ofstream out(dump_path, std::ios::binary);
            size_t total = 0;
            for (auto &v : dumps) { out.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(Cand))); total += v.size(); }
            printf("num_candidates: %zu\n", total);
        }
        std::vector<int32_t> spans;
        const int cover_rc = coverage_depth && !dumping ? write_coverage(e, want_gfa ? &spans : nullptr) : 0;
        const int gfa_rc = want_gfa && !dumping && !cover_rc ? write_gfa(e, spans) : 0;
        const int cons_rc = pileup_depth && !dumping ? write_consensus(e) : 0;
        const int vcf_rc = want_vcf && !dumping && !cons_rc ? write_variants(e) : 0;
        GPU_close(&s, num_threads);
        return cover_rc ? cover_rc : gfa_rc ? gfa_rc : cons_rc ? cons_rc : vcf_rc;
    }

    // per-thread candidate lists, contiguous read ranges like darwin.cpp:619-629
    std::vector<std::vector<Cand> > per_thread(num_threads);
    Tick t_query = now();
    if (!cand_path.empty()) {
        std::vector<Cand> cands;
        std::ifstream in(cand_path, std::ios::binary);
        if (!in) { fprintf(stderr, "cannot open candidates file '%s'\n", cand_path.c_str()); return 1; }
        Cand c;
        while (in.read((char *)&c, sizeof c)) cands.push_back(c);
        const size_t per = (cands.size() + num_threads - 1) / num_threads;
        for (int i = 0; i < num_threads; i++) {
            const size_t lo = std::min(cands.size(), i * per), hi = std::min(cands.size(), lo + per);
            per_thread[i].assign(cands.begin() + lo, cands.begin() + hi);
        }
    } else {
        DsoftIndex index;
        t_stage = now();
        index.build(reference_seqs, dp);
        printf("Reference length: %u, %zu pieces\n", index.reference_length(), reference_seqs.size());
        print_stage("Time elapsed (seed position table construction)", t_stage, now());      // darwin.cpp:596
        t_query = now();
        const int num_reads = (int)reads_seqs.size();
        const int reads_per_thread = (int)std::ceil(1.0 * num_reads / num_threads);
        std::vector<std::thread> filt;
        for (int i = 0; i < num_threads; i++) {
            filt.push_back(std::thread([&, i] {
                const Tick t0 = now();
                const int lo = std::min(num_reads, i * reads_per_thread), hi = std::min(num_reads, lo + reads_per_thread);
                DsoftScratch sc;
                std::vector<DsoftCandidate> f, r;
                for (int k = lo; k < hi; k++) {
                    f.clear(); r.clear();
                    index.query(reads_seqs[k].data(), (uint32_t)reads_seqs[k].size(), k, sc, f);        // darwin.cpp:213
                    index.query(rev_reads_seqs[k].data(), (uint32_t)rev_reads_seqs[k].size(), k, sc, r);  // :252
                    for (const DsoftCandidate &c : f) per_thread[i].push_back(Cand{c.ref_id, c.query_id, c.ref_pos, c.query_pos, 0});
                    for (const DsoftCandidate &c : r) per_thread[i].push_back(Cand{c.ref_id, c.query_id, c.ref_pos, c.query_pos, 1});
                }
                print_stage("Time finding seeds", t0, now());            // darwin.cpp:300
            }));
        }
        for (auto &t : filt) t.join();
    }
    size_t total = 0;
    for (auto &v : per_thread) total += v.size();
    printf("num_candidates: %zu\n", total);
    if (!dump_path.empty()) {
        std::ofstream out(dump_path, std::ios::binary);
        for (auto &v : per_thread) out.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(Cand)));
    }
    if (dsoft_only) return 0;
    if (shard_world > 1) {
        // this rank's share: every W-th candidate of the whole list (chain lengths vary widely),
        // dealt out again in contiguous ranges to its feeder threads
        std::vector<Cand> mine;
        size_t g = 0;
        for (auto &v : per_thread)
            for (const Cand &c : v)
                if ((int)(g++ % (size_t)shard_world) == shard_rank) mine.push_back(c);
        const size_t per = (mine.size() + num_threads - 1) / num_threads;
        for (int i = 0; i < num_threads; i++) {
            const size_t lo = std::min(mine.size(), i * per), hi = std::min(mine.size(), lo + per);
            per_thread[i].assign(mine.begin() + lo, mine.begin() + hi);
        }
    }
    if (recode) {
        const Tick t0 = now();
        recode_in_place(reference_seqs); recode_in_place(reads_seqs); recode_in_place(rev_reads_seqs);
        print_stage("Time converting bases", t0, now());                          // darwin.cpp:405
    }

    if (!gather_id.empty()) return gathered_run(per_thread, gather_id);

    std::vector<GPU_storage> s;
    GPU_init(tile_size, tile_overlap, gap_open, gap_extend, match_score, mismatch_score, tile_size - tile_overlap,
             &s, num_threads);
    std::vector<std::thread> threads;
    for (int i = 0; i < num_threads; i++)
        threads.push_back(std::thread(feeder, i, &per_thread[i], (size_t)0, per_thread[i].size(), s[i]));
    for (auto &t : threads) t.join();
    print_stage("Time elapsed (seed table querying + aligning)", t_query, now());             // darwin.cpp:639
    GPU_close(&s, num_threads);
    return 0;
}
