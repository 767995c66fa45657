"""`ipk build`-compatible command line for the MI355X engine (SURVEY.md section 8f, rows n3 + n4).

Option names and defaults follow the reference wrapper (ipk.py:70-230 -> argv table ipk.py:292-329,
ipk/src/command_line.cpp:83-147), and so does the flow of main.cpp:129-200 for the stages this repository owns:

  reference tree (-t) -> ghost nodes (extended_tree.cpp:76-162; saved as workdir/extended_trees/extended_tree.newick)
  -> AR outputs found by suffix in --ar-dir (ar.cpp:611-640: *.raxml.ancestralProbs, *.raxml.ancestralTree)
  -> AR tree rerooted if the reference tree is rooted (main.cpp:172-178) -> extended/AR node mapping (ar.cpp:790-834)
  -> ghost groups (db_builder.cpp:495-553) -> GPU scoring -> filter (MIF0 or random, on the device) -> database file.

Alignment reduction/extension and RUNNING the ancestral reconstruction are IPK's host stages and out of scope
(DESIGN.md): their options are accepted for command-line compatibility and ignored; the AR outputs must exist (e.g. from
`ipk.py build --ar-only` of the reference, or raxml-ng run on the saved extended tree).

  ipk.py build -r aln.fasta -t tree.nwk -w work --ar-dir work/AR -k 10
  ipk.py diff [-v] [--eps 1e-2 | --exact] A.ipk B.ipk          (the reference's ipkdiff; exit status 1 on a difference)
  ipk.py dump [--limit N] DB.ipk                               (the reference's ipkdump)
  ipk.py place -i DB.ipk -q reads.fasta [-o out.tsv]            (this engine's: the reads' k-mers looked up and summed per branch)
  ipk.py merge -o OUT.ipk [--on device|host] SHARD.ipk ...     (shard files with disjoint k-mer sets joined into one database file)
  ipk.py build ... --group-range LO:HI -o SHARD.ipk            (a branch shard: only the branch groups LO <= i < HI are scored)
  ipk.py merge --shared-keys -o OUT.ipk SHARD.ipk ...          (branch shards, whose k-mer sets overlap, joined and filtered anew)

--mapping (optional, not in the reference): TSV `ar_node_label <TAB> branch_postorder_id` per ghost node in scoring order;
replaces the tree-derived plan (synthetic inputs without trees).
"""
import glob
import os
import sys
import time

import click
import numpy as np


@click.group()
def ipk():
    """MI355X phylo-k-mer database builder (drop-in for the scoring path of IPK)."""


@ipk.command()
@click.option("-b", "--ar", type=click.Path(), help="(ignored) ancestral-reconstruction binary; use --ar-dir")
@click.option("-r", "--refalign", type=click.Path(), help="(ignored here) reference alignment")
@click.option("-t", "--reftree", type=click.Path(), help="reference tree (newick); stored in the database header")
@click.option("-s", "--states", type=click.Choice(["nucl", "amino"]), default="nucl", show_default=True)
@click.option("-v", "--verbosity", type=int, default=1, show_default=True)
@click.option("-w", "--workdir", required=True, type=click.Path(file_okay=False))
@click.option("--write-reduction", type=click.Path(), help="(ignored)")
@click.option("-a", "--alpha", type=float, default=1.0, show_default=True, help="(ignored) AR gamma shape")
@click.option("-c", "--categories", type=int, default=4, show_default=True, help="(ignored) AR rate categories")
@click.option("-k", "--k", "k", type=int, default=8, show_default=True,
              help="k-mer length (DNA <= 16, AA <= 6 on this engine; DNA k = 15, 16 are built in key-range passes, on one GPU)")
@click.option("-m", "--model", default=None, help="(ignored) AR model")
@click.option("--convert-uo", is_flag=True, help="(ignored)")
@click.option("--no-reduction", is_flag=True, help="(ignored)")
@click.option("--reduction-ratio", type=float, default=0.99, show_default=True, help="(ignored)")
@click.option("--omega", type=float, default=1.5, show_default=True, help="score threshold (omega/#states)^k")
@click.option("--filter", "filter_", type=click.Choice(["mif0", "random"]), default="mif0", show_default=True,
              help="k-mer order of the file: mif0 (filter.cpp:55-119) or random -- this engine's fixed draw per k-mer code, not the "
                   "reference's engine in hash-map order; both run on the device and feed the streamed device writer")
@click.option("-u", "--mu", type=float, default=1.0, show_default=True, help="(parsed, unused -- as in the reference build)")
@click.option("--ghosts", type=click.Choice(["inner-only", "outer-only", "both"]), default="both", show_default=True)
@click.option("--use-unrooted", is_flag=True, help="(ignored)")
@click.option("--merge-branches", is_flag=True, help="unsupported (as in the reference, main.cpp:31-37)")
@click.option("--ar-dir", type=click.Path(exists=True, file_okay=False), default=None,
              help="directory holding <prefix>.raxml.ancestralProbs / .raxml.ancestralTree [searched in the workdir if absent]")
@click.option("--ar-only", is_flag=True, help="(ignored)")
@click.option("--ar-config", type=click.Path(), help="(ignored)")
@click.option("--keep-positions", is_flag=True,
              help="(ipk-aa-pos; amino acids) every database entry carries the window position of its kept score "
                   "(db_builder.cpp:655-662,687-689): the position rides along through the one scoring pass on the device "
                   "(ipkgpu_score_groups_keymajor_positions_device; several ranks: the positions travel through the k-mer-keyed exchange beside "
                   "their entries); the entry layout (branch, score, u16 position) is a guess like the rest of the file")
@click.option("--uncompressed", is_flag=True, help="(ignored, as in the reference)")
@click.option("--threads", type=int, default=0,
              help="host threads of the probability loader [0 = every core this process may run on, divided among the ranks of a node; the reference's --threads only "
                   "feeds the AR tool (ar.cpp:669,749), which this command does not run]")
@click.option("-o", "--output", default=None, help="output file [workdir/DB.ipk]")
@click.option("--on-disk", is_flag=True,
              help="build a database that does not fit device memory: the groups are scored in pieces, every piece's result leaves the device "
                   "split into 32 k-mer-keyed batches under workdir/hashmaps, and the batches are merged, filtered and written one at a time "
                   "(db_builder.cpp:340-458); same file as the default build, slower, bound by the file system; one GPU, no --keep-positions, "
                   "k <= 14 (amino acids 6)")
@click.option("--mapping", type=click.Path(exists=True), default=None,
              help="TSV: AR node label <TAB> branch post-order id, one line per ghost node (instead of the tree-derived plan)")
@click.option("--num-tree-nodes", type=int, default=0, help="node count of the original tree (MIF0's N, db_builder.cpp:261); default: the reference tree's, or branch groups + 1 with --mapping")
@click.option("--device", type=int, default=None, help="GPU index [0; LOCAL_RANK under torchrun]")
@click.option("--key-passes", type=int, default=None,
              help="build the database in this many key-range passes (4^j; DNA k = 14..16), one pass' k-mers in device memory at a "
                   "time [auto: one call up to k = 14, 4^(k-14) passes above]")
@click.option("--union-on-device", is_flag=True,
              help="key-range builds only: every pass' filtered database stays on the GPU, after the last pass they are united there "
                   "(ipkgpu_db_union) and written once -- no pass files, no host merge; same file.  What does not fit device memory "
                   "falls back to pass files and the host merge")
@click.option("--group-range", default=None, metavar="LO:HI",
              help="score only the branch groups at positions LO <= i < HI of the first-seen group order and write them as an ordinary "
                   "database file, a branch shard (MIF0's N stays the whole tree's); `merge --shared-keys` joins the shards of all "
                   "ranges, in range order, into the file of the whole build.  One GPU, no --on-disk, no key-range passes")
def build(ar, refalign, reftree, states, verbosity, workdir, write_reduction, alpha, categories, k, model, convert_uo,
          no_reduction, reduction_ratio, omega, filter_, mu, ghosts, use_unrooted, merge_branches, ar_dir, ar_only,
          ar_config, keep_positions, uncompressed, threads, output, on_disk, mapping, num_tree_nodes, device, key_passes,
          union_on_device, group_range):
    """Computes a database of phylo-k-mers from precomputed ancestral probabilities."""
    import ipk_amd
    from ipk_amd import dbfile, distributed, keyrange, ondisk
    from ipk_amd.loader import AncestralProbs

    if keep_positions and states == "nucl":
        raise click.UsageError("--keep-positions is not supported for DNA.")              # ipk.py:281-282
    if merge_branches:
        raise click.UsageError("--merge-branches is not supported (the reference only guards it, main.cpp:31-37)")
    from ipk_amd import tree as T
    sigma = 4 if states == "nucl" else 20
    if not 2 <= k <= ipk_amd.max_k_keyrange(sigma):
        raise click.UsageError(f"k must be in [2, {ipk_amd.max_k_keyrange(sigma)}] for --states {states} on this engine")
    # k beyond one call's key space (DNA 15, 16) or --key-passes: key-range passes (ipk_amd/keyrange.py), one process
    use_passes = k > ipk_amd.max_k(sigma) or key_passes is not None
    if use_passes and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise click.UsageError(f"k = {k} / --key-passes: key-range passes run on ONE GPU (several ranks: k <= {ipk_amd.max_k(sigma)})")
    if use_passes:
        try:
            keyrange.plan(sigma, k, key_passes)
        except ValueError as e:
            raise click.UsageError(f"--key-passes: {e}")
    if union_on_device and not use_passes:
        raise click.UsageError(f"--union-on-device goes with key-range passes (DNA k > {ipk_amd.max_k(4)}, or --key-passes): other builds write no pass files")
    if on_disk and keep_positions:
        raise click.UsageError("--on-disk does not keep positions (neither does the reference, db_builder.cpp:469): drop --keep-positions or --on-disk")
    if on_disk and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise click.UsageError("--on-disk runs on ONE GPU: the batches inside a rank's shard would need a slot mapping of their own (not built)")
    if on_disk and use_passes:
        raise click.UsageError(f"--on-disk is not combined with key-range passes (k = {k} / --key-passes): a pass already bounds device memory")
    if group_range is not None:
        group_range = _parse_group_range(group_range)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise click.UsageError("--group-range runs on ONE GPU: give every process its own range and join the files with `merge --shared-keys`")
        if on_disk:
            raise click.UsageError("--group-range is not combined with --on-disk")
        if use_passes:
            raise click.UsageError(f"--group-range is not combined with key-range passes (k = {k} / --key-passes)")
    os.makedirs(workdir, exist_ok=True)
    output = output or os.path.join(workdir, "DB.ipk")

    def find_by_suffix(suffix):                                                       # ar.cpp:458-469, :611-640
        dirs = [ar_dir] if ar_dir else [os.path.join(workdir, "extended_trees"), os.path.join(workdir, "AR"), workdir]
        for d in dirs:
            hits = sorted(glob.glob(os.path.join(d, "*" + suffix)))
            if hits:
                return hits[0]
        raise click.UsageError(f"Could not find \"*{suffix}\" in {dirs}: this build does not run the ancestral reconstruction itself")

    probs_file = find_by_suffix(".raxml.ancestralProbs")
    orig = ext = None
    tree_index, newick, n_tree_nodes = [], "", 0
    if reftree:
        orig = T.Tree.load(reftree)
        if not orig.is_rooted and not use_unrooted:                                   # extended_tree.cpp:169-177
            raise click.UsageError("This reference tree is not rooted. Please provide a rooted tree or provide --use-unrooted. "
                                   "WARNING! This may impact placement accuracy.")
        tree_index, newick, n_tree_nodes = orig.index(), orig.newick(), orig.num_nodes
    labels, branches = [], []
    if mapping:
        for line in open(mapping):
            line = line.rstrip("\n")
            if not line or line.startswith("#"):
                continue
            lab, br = line.split("\t")[:2]
            if ghosts == "inner-only" and not lab.endswith("_X0"):
                continue
            if ghosts == "outer-only" and not lab.endswith("_X1"):
                continue
            labels.append(lab); branches.append(int(br))
    else:
        if orig is None:
            raise click.UsageError("-t/--reftree is required (or --mapping for inputs without trees)")
        ext = orig.extend()
        ext_dir = os.path.join(workdir, "extended_trees")                               # main.cpp:39-46
        os.makedirs(ext_dir, exist_ok=True)
        if int(os.environ.get("RANK", "0")) == 0:
            with open(os.path.join(ext_dir, "extended_tree.newick"), "w") as fh:
                fh.write(ext.newick() + "\n")
        ar_tree = T.Tree.load(find_by_suffix(".raxml.ancestralTree"))
        if orig.is_rooted and not ar_tree.is_rooted:                                   # main.cpp:172-178
            ar_tree.reroot()
        for _ext_label, ar_label, branch in T.ghost_plan(orig, ext, ar_tree, ghosts):
            labels.append(ar_label); branches.append(branch)
    if not labels:
        raise click.UsageError("no ghost nodes selected")

    # several GPUs: one process per GPU (torchrun); branch groups are split into contiguous ranges of the group
    # order, every rank scores its range, the k-mer-keyed exchange (RCCL) leaves rank r with the k-mers code % P == r
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dist = None
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(device)
        own_group = not dist.is_initialized()
        if own_group:
            dist.init_process_group(os.environ.get("IPK_DIST_BACKEND", "nccl"))
    all_branches = list(branches)
    group_order = list(dict.fromkeys(all_branches))                        # first-seen order (db_builder.cpp:524-553)
    g0, g1 = distributed.shard_range(len(group_order), world, rank)
    if group_range is not None:
        g0, g1 = group_range
        if g1 > len(group_order):
            raise click.UsageError(f"--group-range {g0}:{g1}: there are {len(group_order)} branch groups")
    mine = set(group_order[g0:g1])
    sel = [i for i, b in enumerate(all_branches) if b in mine]
    labels, branches = [labels[i] for i in sel], [all_branches[i] for i in sel]

    t0 = time.time()
    arp = AncestralProbs(probs_file, sigma)
    mats = arp.read(labels, n_threads=threads if threads > 0 else max(1, len(os.sched_getaffinity(0)) // world)) if labels else np.zeros((0, arp.sites, sigma), np.float32)
    t_load = time.time() - t0
    log_eps = ipk_amd.log_threshold(omega, sigma, k)
    eng = ipk_amd.Engine(device)
    # the reference's command computes every window (its lists live in host memory): a DNA k >= 13 window whose half list exceeds
    # the big-list kernels' capacity is scored slice by slice instead of ending the build (no effect at other k)
    eng.set_option("slice_long_lists", 1)
    if use_passes:
        n_nodes = num_tree_nodes or n_tree_nodes or len(group_order) + 1
        kr = keyrange.build_db_file(eng, mats, np.array(branches, dtype=np.uint32), k, log_eps, sigma, output, workdir,
                                    "DNA", tree_index, newick, omega, filter_, n_nodes, key_passes, union_on_device=union_on_device)
        if verbosity:
            # the reference's three stage timers (db_builder.cpp:236,290,336), summed over the passes
            n = kr["passes"]
            click.echo(f"Loaded {len(labels)} node matrices ({arp.sites} sites) in {t_load * 1e3:.0f} ms")
            click.echo(f"Computation time: {kr['score_s'] * 1e3:.0f} ms ({kr['emitted']} scored phylo-k-mers; {n} key-range passes)")
            click.echo(f"Filtering time: {kr['filter_s'] * 1e3:.0f} ms ({n} key-range passes)")
            if kr["route"] == "device":
                click.echo(f"Merge time: {(kr['write_s'] + kr['union_s']) * 1e3:.0f} ms ({n} pass databases united on the device, one file written)")
            else:
                click.echo(f"Merge time: {(kr['write_s'] + kr['merge_s']) * 1e3:.0f} ms ({n} pass files written and merged"
                           + ("; --union-on-device did not fit device memory)" if kr["route"] == "fallback" else ")"))
            click.echo(f"Output: {output} ({kr['totals'][0]} k-mers, {kr['totals'][1]} entries)")
        eng.close(); arp.close()
        return
    if on_disk:
        n_nodes = num_tree_nodes or n_tree_nodes or len(group_order) + 1
        od = ondisk.build_db_file(eng, mats, np.array(branches, dtype=np.uint32), k, log_eps, sigma, output, workdir,
                                  "DNA" if sigma == 4 else "AA", tree_index, newick, omega, filter_, n_nodes)
        if verbosity:
            # the reference's three stage timers (db_builder.cpp:236,290,336) over the on-disk build's three stages
            click.echo(f"Loaded {len(labels)} node matrices ({arp.sites} sites) in {t_load * 1e3:.0f} ms")
            click.echo(f"Computation time: {od['stage1_s'] * 1e3:.0f} ms ({od['emitted']} scored phylo-k-mers; {od['pieces']} pieces of groups spilled "
                       f"in {od['batches']} batches, {od['spilled_bytes']} bytes)")
            click.echo(f"Filtering time: {od['stage2_s'] * 1e3:.0f} ms ({od['batches']} batches merged, filtered and written; device memory held: "
                       f"at most {od['held_peak']} of {od['budget_bytes']} bytes)")
            click.echo(f"Merge time: {od['stage3_s'] * 1e3:.0f} ms ({od['batches']} batch files merged)")
            click.echo(f"Output: {output} ({od['totals'][0]} k-mers, {od['totals'][1]} entries)")
        eng.close(); arp.close()
        return
    t0 = time.time()
    if world > 1:
        import torch
        mats = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    db, parts = distributed.build_db_shard(eng, mats, np.array(branches, dtype=np.uint32), k, log_eps, sigma, dist, world, rank,
                                           positions=keep_positions)
    t_score = time.time() - t0
    # MIF0's N = _original_tree.get_node_count() (db_builder.cpp:261); without a tree: groups = the non-root nodes (:524-553)
    n_nodes = num_tree_nodes or n_tree_nodes or len(group_order) + 1
    seq_name = "DNA" if sigma == 4 else "AA"
    stage = {}

    def write_shard(file):
        # one filter stage and one writer for every filter, plain and --keep-positions (`db` then carries positions and the device
        # writer packs the positioned records): the filter on the device, the records packed there in filter order and streamed
        # to the file (ipkgpu_db_write) -- the database itself on one GPU, this rank's shard on several (a shard's header carries
        # only its totals).  --filter random is this engine's draw, one fixed value per k-mer CODE (ipkgpu.h), not the reference's
        # (filter.cpp:122-145), so the file does not depend on how the k-mers are sharded.
        one = world == 1
        stage["filter_s"], stage["write_s"] = dbfile.filter_and_write_device(
            eng, db, file, filter_, seq_name, tree_index if one else [], newick if one else "", k, omega, n_nodes,
            ipk_amd.score_threshold(omega, sigma, k))
    t0 = time.time()
    totals = distributed.write_db_file(output, seq_name, tree_index, newick, k, omega, write_shard, workdir, dist, world, rank)
    if world == 1:
        totals = (db.num_keys, db.num_entries)
    t_filter = stage["filter_s"]
    t_write = time.time() - t0 - t_filter                            # the shard's write and, on several ranks, the merge of the shard files
    emitted = parts.emitted
    if world > 1:
        import torch
        e = torch.tensor([emitted], dtype=torch.int64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(e)
        emitted = int(e.item())
    if verbosity and rank == 0:
        # the reference prints the same three stage timers (db_builder.cpp:236,290,336)
        click.echo(f"Loaded {len(labels)} node matrices ({arp.sites} sites) in {t_load * 1e3:.0f} ms" + (f" on each of {world} ranks" if world > 1 else ""))
        click.echo(f"Computation time: {t_score * 1e3:.0f} ms ({emitted} scored phylo-k-mers)")
        click.echo(f"Filtering time: {t_filter * 1e3:.0f} ms")
        click.echo(f"Merge time: {t_write * 1e3:.0f} ms")
        click.echo(f"Output: {output} ({totals[0]} k-mers, {totals[1]} entries)")
        click.echo("Note: the database layout is a reconstruction of i2l's Boost binary archive (i2l and Boost are not part of the "
                   "reference tree): UNPINNED against a real .ipk -- ipk_amd/csrc/ipk_format.hpp is the one file that knows the bytes; "
                   "IPKGPU_BOOST_ARCHIVE_VERSION sets the archive's library version (default 19).  Guessed fields: the protocol-version "
                   "word behind the archive preamble and the positions flag behind the sequence type (position, width, value; "
                   f"IPKGPU_IPK_PROTOCOL_VERSION, now {dbfile.protocol_version()}, 0 = both left out), the widths of the tree index "
                   "(u64 / f64), filter value (f32) and key (u32)" + (", and the u16 window position of a positioned entry." if keep_positions else "."))
    db.free(); parts.free(); eng.close(); arp.close()
    if world > 1 and own_group:
        dist.destroy_process_group()


# ---- looking into database files: the reference's tools ipkdiff / ipkdump (tools/src/diff.cpp, tools/src/dump.cpp) -----------------

_ALPHABET = {"DNA": ("ACGT", 2), "AA": ("RHKDESTNQCGPAILMFWYV", 5)}       # IPK's code order (AA: ar.cpp:227-234), bits per symbol


def decode_kmer(key, k, sequence_type):
    """i2l::decode_kmer: the k symbols of a packed code, first symbol in the highest bits (pk_compute.cpp:96-104)."""
    letters, bits = _ALPHABET[sequence_type]
    return "".join(letters[(int(key) >> (bits * (k - 1 - i))) & ((1 << bits) - 1)] for i in range(k))


def preorder_ids(newick):
    """post-order id -> pre-order id (root 0, children in file order) of the header's tree."""
    from ipk_amd import tree as T
    t = T.Tree.parse(newick)
    n = t.num_nodes
    kids = [[] for _ in range(n)]
    root = n - 1
    for i in range(n):
        p = t.parent(i)
        if p < 0:
            root = i
        else:
            kids[p].append(i)                      # (ascending post-order id = file order among siblings)
    pre, stack, nxt = [0] * n, [root], 0
    while stack:
        v = stack.pop()
        pre[v] = nxt
        nxt += 1
        stack.extend(reversed(kids[v]))
    t.close()
    return pre


def _g(x):
    return "%g" % x                                 # what `std::cout << double` prints


@ipk.command()
@click.option("-v", "--verbose", is_flag=True, help="also print the differing (k-mer, branch) pairs: code, k-mer, branch, 10^A, 10^B ('-' = not scored)")
@click.option("--eps", type=float, default=1e-2, show_default=True, help="scores match iff |a - b| < eps (the reference's constant, diff.cpp:212)")
@click.option("--exact", is_flag=True, help="scores match iff their bits are equal (eps = 0)")
@click.option("--max-records", type=int, default=100, show_default=True, help="with -v: print at most this many pairs (the counts are exact anyway)")
@click.option("--stream", is_flag=True, help="compare by key ranges, neither file ever on the GPU whole: for files that do not fit device memory")
@click.option("--budget-mib", type=float, default=None, help="with --stream: the device memory (MiB) the comparison may use on top of what the engine holds [what is free]")
@click.option("--device", type=int, default=0, show_default=True, help="GPU index")
@click.argument("a", type=click.Path(exists=True, dir_okay=False))
@click.argument("b", type=click.Path(exists=True, dir_okay=False))
def diff(verbose, eps, exact, max_records, stream, budget_mib, device, a, b):
    """Compares two database files (the reference's ipkdiff): both are loaded onto the GPU and compared there.

    Prints the reference's lines in its order, tab separated, each with OK or DIFF and the two values.  Deviations from the
    reference's tool: `Tree index` is really compared (the reference prints ???); `Position support` is printed (commented out there);
    two positioned files also get a `Phylo-k-mer positions` line (equal scores, different positions); the k-mers of the verbose list
    come in ascending order; and the exit status is 1 when any line says DIFF -- the reference's ipkdiff always returns 0
    (diff.cpp:115-116).

    --stream prints the same text and returns the same status without loading either file whole: the head lines come from the files'
    heads, the comparison from ipkgpu_db_diff_files -- key ranges that each fit the device (or --budget-mib), one histogram pass over
    each file to plan them and one pass per range (include/ipkgpu.h)."""
    import ipk_amd
    from ipk_amd import dbfile
    if budget_mib is not None and not stream:
        raise click.UsageError("--budget-mib goes with --stream")
    if budget_mib is not None and not budget_mib > 0:
        raise click.UsageError("--budget-mib must be positive")
    eng = ipk_amd.Engine(device)
    try:
        if stream:
            da = db_ = None
            ha, hb = dbfile.file_info(a), dbfile.file_info(b)
        else:
            da, db_ = eng.load_db(a), eng.load_db(b)
            ha, hb = da.header, db_.header
        all_ok = True

        def line(name, va, vb, match=None, show=True):
            nonlocal all_ok
            match = (va == vb) if match is None else match
            all_ok &= bool(match)
            click.echo(f"{name}:\t{'OK' if match else 'DIFF'}\t" + (f"{va}\t{vb}" if show else " \t "))

        def log_eps(h):
            sigma = {"DNA": 4, "AA": 20}.get(h["sequence_type"])
            return _g(ipk_amd.log_threshold(h["omega"], sigma, h["kmer_size"])) if sigma and h["kmer_size"] else "?"

        line("Sequence type", ha["sequence_type"], hb["sequence_type"])
        line("Position support", str(ha["positions_loaded"]).lower(), str(hb["positions_loaded"]).lower())
        line("Protocol version", ha["protocol_version"], hb["protocol_version"])
        line("k-mer size", ha["kmer_size"], hb["kmer_size"])
        same_omega = ha["omega"] == hb["omega"]
        line("Omega", _g(ha["omega"]), _g(hb["omega"]), same_omega)
        line("Threshold", log_eps(ha), log_eps(hb), same_omega and ha["kmer_size"] == hb["kmer_size"] and ha["sequence_type"] == hb["sequence_type"])
        line("Reference tree", None, None, ha["newick"] == hb["newick"], show=False)
        line("Tree index", len(ha["tree_index"]), len(hb["tree_index"]), ha["tree_index"] == hb["tree_index"])
        if stream:
            if budget_mib is not None:
                eng.set_option("release_workspaces", 1)
                eng.set_option("device_budget_bytes", eng.mem_stats()[0] + int(budget_mib * (1 << 20)))
            c, rec, _ = eng.diff_files(a, b, eps=0.0 if exact else eps, max_records=max_records if verbose else 0)
        else:
            c, rec = eng.diff_dbs(da, db_, eps=0.0 if exact else eps, max_records=max_records if verbose else 0)
        line("Number of k-mers", c["keys_a"], c["keys_b"])
        line("Number of phylo-k-mers", c["entries_a"], c["entries_b"])
        n_diffs = c["entries_only_a"] + c["entries_only_b"] + c["scores_differ"]
        all_ok &= n_diffs == 0
        click.echo(f"Phylo-k-mer scores:\t{'OK' if n_diffs == 0 else 'DIFF'}\t{n_diffs}")
        if ha["positions_loaded"] and hb["positions_loaded"]:
            all_ok &= c["positions_differ"] == 0
            click.echo(f"Phylo-k-mer positions:\t{'OK' if c['positions_differ'] == 0 else 'DIFF'}\t{c['positions_differ']}")
        if verbose:
            click.echo("\t\tcode\tk-mer\tbranch\tA score\tB score")
            k, st = ha["kmer_size"], ha["sequence_type"]
            val = lambda x: "-" if np.isnan(x) else _g(10.0 ** float(x))
            for r in rec:
                kmer = decode_kmer(r["key"], k, st) if st in _ALPHABET else "?"
                click.echo(f"\t\t{int(r['key'])}\t{kmer}\t{int(r['branch'])}\t{val(r['a_score'])}\t{val(r['b_score'])}\t")
        if not stream:
            da.free(); db_.free()
    finally:
        eng.close()
    sys.exit(0 if all_ok else 1)


def _parse_group_range(text):
    """LO:HI -> (lo, hi): decimal integers, 0 <= LO < HI."""
    try:
        lo, hi = (int(x) for x in text.split(":"))
    except ValueError:
        raise click.UsageError(f"--group-range takes LO:HI, two integers, not '{text}'")
    if not 0 <= lo < hi:
        raise click.UsageError("--group-range needs 0 <= LO < HI")
    return lo, hi


def _parse_key_range(text):
    """LO:HI -> (lo, hi): integers (0x.. allowed), 0 <= LO <= HI <= 2^32."""
    try:
        lo, hi = (int(x, 0) for x in text.split(":"))
    except ValueError:
        raise click.UsageError(f"--key-range takes LO:HI, two integers, not '{text}'")
    if not 0 <= lo <= hi <= 1 << 32:
        raise click.UsageError("--key-range needs 0 <= LO <= HI <= 2^32")
    return lo, hi


@ipk.command()
@click.option("--limit", type=int, default=None, help="print only the first N k-mers of the file [all]")
@click.option("--key-range", default=None, metavar="LO:HI", help="print only the k-mers with LO <= code < HI, the file streamed through the GPU and never held whole")
@click.option("--device", type=int, default=0, show_default=True, help="GPU index")
@click.argument("db", type=click.Path(exists=True, dir_okay=False))
def dump(limit, key_range, device, db):
    """Prints a database file as text (the reference's ipkdump), in the file's record order.

    Per k-mer one line with the decoded k-mer, then one line per entry: TAB 10^score (as %g) TAB pre-order id of the branch in the
    header's tree (root 0, children in file order), and TAB window position for a positioned file.  A file without a tree in its
    header (a shard) prints the branch's post-order id as stored.

    --key-range LO:HI prints the records of that key range, in file order among themselves (ipkgpu_db_load_key_range); a file that does
    not fit device memory is dumped range by range this way.  Its dump as a whole, in file order, is not supported: the file's order
    is the filter's, not the keys', and no range of keys is a stretch of it."""
    import ipk_amd
    eng = ipk_amd.Engine(device)
    try:
        d = eng.load_db(db, key_range=_parse_key_range(key_range)) if key_range is not None else eng.load_db(db)
        h = d.header
        pre = preorder_ids(h["newick"]) if h["newick"] else None
        keys, off, order = d.keys(), d.key_offsets(), d.filter_order()
        br, sc = d.entries()
        pos = d.positions()
        out = []
        for i in (order if limit is None else order[:max(limit, 0)]):
            out.append(decode_kmer(keys[i], h["kmer_size"], h["sequence_type"]))
            for j in range(int(off[i]), int(off[i + 1])):
                b = int(br[j])
                node = pre[b] if pre is not None and b < len(pre) else b
                out.append(f"\t{_g(10.0 ** float(sc[j]))}\t{node}" + (f"\t{int(pos[j])}" if pos is not None else ""))
        click.echo("\n".join(out))
        d.free()
    finally:
        eng.close()


# ---- placement: what a database is for ---------------------------------------------------------------------------------------------

def read_fasta(text):
    """[(name, sequence)] of FASTA text: records may span lines, the name is the header's text up to the first blank, and '-', '.' and
    whitespace are dropped from the sequence.  Lines before the first header are ignored."""
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            words = line[1:].split()
            out.append((words[0] if words else "", []))
        elif out:
            out[-1][1].append("".join(ch for ch in line if not ch.isspace() and ch not in "-."))
    return [(name, "".join(parts)) for name, parts in out]


def placement_lines(names, res, keep_factor, with_strand=False):
    """The TSV lines of `ipk.py place` for a Placements: per query its placements best first while lwr >= keep_factor x the best's
    lwr -- query, branch, score (%.9g: the float's bits), count, n_kmers, lwr (%.17g); a query without placements: one line of '-'.
    with_strand: a seventh column, '+' (the strand given) or '-' (its reverse complement was placed)."""
    from ipk_amd.engine import PLACE_NONE
    lines = []
    tail = (lambda i: "\t-" if res.strand[i] else "\t+") if with_strand else (lambda i: "")
    for i, name in enumerate(names):
        kept = 0
        for j in range(res.keep):
            if int(res.branches[i, j]) == PLACE_NONE or res.lwr[i, j] < keep_factor * res.lwr[i, 0]:
                break
            lines.append(f"{name}\t{int(res.branches[i, j])}\t{float(res.scores[i, j]):.9g}\t{int(res.counts[i, j])}\t{int(res.n_kmers[i])}\t"
                         f"{float(res.lwr[i, j]):.17g}" + tail(i))
            kept += 1
        if kept == 0:
            lines.append(f"{name}\t-\t-\t-\t{int(res.n_kmers[i])}\t-" + tail(i))
    return lines


def _check_selection(db_path, mu, omega):
    """Refuses, with a message, a --mu outside [0, 1] and an --omega below the file's (entries under the build's threshold are not in
    the file, so a lower omega cannot be served)."""
    from ipk_amd import dbfile
    if mu is not None and not 0.0 <= mu <= 1.0:
        raise click.UsageError(f"--mu must be in [0, 1], not {mu}")
    if omega is not None:
        file_omega = dbfile.file_info(db_path)["omega"]
        if not np.float32(omega) >= np.float32(file_omega):          # binary32, as the file stores it: the build's own --omega is not below it
            raise click.UsageError(f"--omega {_g(omega)} is below the file's omega {_g(file_omega)}: entries under the build's threshold "
                                   "are not in the file")


@ipk.command()
@click.option("-i", "--input", "db_path", required=True, type=click.Path(exists=True, dir_okay=False), help="database file (of this engine's builds)")
@click.option("-o", "--output", required=True, help="the selection's database file")
@click.option("--mu", type=float, default=None, help="keep the first fraction MU of the file's k-mers in filter order [all]")
@click.option("--omega", type=float, default=None, help="keep the entries above this omega's threshold; becomes the output's omega [the file's]")
@click.option("--queries", default=None, type=click.Path(exists=True, dir_okay=False),
              help="keep only the k-mers these query sequences (FASTA) can look up: the restriction that places them as the whole file does")
@click.option("--expand-ambiguous", is_flag=True, default=False, help="with --queries: the k-mers `place --expand-ambiguous` looks up")
@click.option("--strands", type=click.Choice(["given", "both"]), default="given", show_default=True, help="with --queries: the k-mers of both strands")
@click.option("--key-range", default=None, metavar="LO:HI", help="keep the k-mers with LO <= code < HI, each with every entry (no other selection goes with it)")
@click.option("--device", type=int, default=0, show_default=True, help="GPU index")
def subset(db_path, output, mu, omega, queries, expand_ambiguous, strands, key_range, device):
    """Writes a selection of a database file as a database file: the first fraction --mu of its k-mers in filter order, of those
    the entries above --omega's threshold (ipkgpu_db_load_select; the definition is in include/ipkgpu.h and is this engine's own --
    the reference's load(file, mu, omega) could not be read).  The file is loaded as far as the selection needs, selected on the GPU
    and written by the device writer; the head is the input's with the new totals and, if given, the new omega.

    --queries restricts the selection to the k-mers the reads of a FASTA file can look up (ipkgpu_db_load_wanted: the file is streamed
    through the GPU in windows and never held whole): `place` of those reads on the output gives what it gives on the input.

    --key-range LO:HI writes the records of that key range as a file (ipkgpu_db_load_key_range, streamed the same way)."""
    import ipk_amd
    from ipk_amd import dbfile
    if key_range is not None and (mu is not None or omega is not None or queries is not None):
        raise click.UsageError("--key-range goes with no other selection")
    _check_selection(db_path, mu, omega)
    eng = ipk_amd.Engine(device)
    try:
        if key_range is not None:
            d = eng.load_db(db_path, key_range=_parse_key_range(key_range))
            dbfile.write_db_device(eng, d, output, **dbfile.header_args(d.header))
            click.echo(f"Output: {output} ({d.num_keys} k-mers, {d.num_entries} entries)")
            d.free()
            return
        wanted = None
        if queries is not None:
            info = dbfile.file_info(db_path)
            with open(queries) as fh:
                seqs = [s for _, s in read_fasta(fh.read())]
            wanted = eng.kmer_set(seqs, {"DNA": 4, "AA": 20}.get(info["sequence_type"], 0), info["kmer_size"], ambiguity=expand_ambiguous, strands=strands)
        d = eng.load_db(db_path, mu=1.0 if mu is None else mu, omega=omega, wanted=wanted)
        head = dbfile.header_args(d.header)
        if omega is not None:
            head["omega"] = omega
        dbfile.write_db_device(eng, d, output, **head)
        click.echo(f"Output: {output} ({d.num_keys} k-mers, {d.num_entries} entries)")
        d.free()
    finally:
        eng.close()


@ipk.command()
@click.option("-i", "--input", "db_paths", required=True, multiple=True, type=click.Path(exists=True, dir_okay=False),
              help="database file (of this engine's builds); repeated: shard files with disjoint k-mer sets, united on the GPU")
@click.option("-q", "--queries", required=True, type=click.Path(exists=True, dir_okay=False), help="query sequences (FASTA)")
@click.option("-o", "--output", default=None, help="output TSV [standard output]")
@click.option("--keep-at-most", type=click.IntRange(1, 64), default=7, show_default=True, help="placements kept per query at most")
@click.option("--keep-factor", type=float, default=0.01, show_default=True, help="a placement is kept while its lwr >= this x the best one's")
@click.option("--expand-ambiguous", is_flag=True, default=False,
              help="expand a k-mer with one ambiguous symbol (N, R, Y, ...; amino acids B, Z, J, X) into its resolutions")
@click.option("--strands", type=click.Choice(["given", "both"]), default="given", show_default=True,
              help="both: place the reverse complement too (DNA) and keep the better strand; adds a seventh column, + or -")
@click.option("--mu", type=float, default=None, help="place on the first fraction MU of the file's k-mers in filter order only [all]")
@click.option("--omega", type=float, default=None, help="place at this omega: entries at or below its threshold are left out [the file's]")
@click.option("--stream-db", is_flag=True, default=False,
              help="never hold the file on the GPU: stream it in windows and keep only the k-mers the queries look up (same output)")
@click.option("--query-batch", type=click.IntRange(1), default=None, help="with --stream-db: queries per pass over the file [all]")
@click.option("--shared-keys", is_flag=True, default=False,
              help="several -i are branch shards whose k-mer sets may overlap: joined on the GPU in the order given and filtered with MIF0")
@click.option("--num-tree-nodes", type=int, default=0, help="with --shared-keys: MIF0's N [the node count of the first shard's tree index]")
@click.option("--device", type=int, default=0, show_default=True, help="GPU index")
def place(db_paths, queries, output, keep_at_most, keep_factor, expand_ambiguous, strands, mu, omega, stream_db, query_batch, shared_keys, num_tree_nodes, device):
    """Places query sequences on a database: the database is loaded onto the GPU, every read's k-mers are looked up there and each
    branch's scores summed (ipkgpu_db_place; the definition is in include/ipkgpu.h).

    One TSV line per kept placement: query, branch, score, count, n_kmers, lwr -- branch is the stored post-order id (what `dump`
    prints for a file without a tree), score the log10 score with the threshold standing in for the query's k-mers the branch does
    not score, count those it does, n_kmers the query's valid k-mers.  By default the given strand only, and symbols outside the
    alphabet (N, X, ...) end a k-mer; --expand-ambiguous and --strands both change that (ipkgpu_db_place_opts in include/ipkgpu.h).

    --mu / --omega load a selection of the file (ipkgpu_db_load_select: only the prefix of the file that holds the first k-mers is
    read) and place on it, at --omega's threshold; what `subset` with the same options writes places alike.

    --stream-db is for a file that does not fit the GPU's memory: per --query-batch queries the file goes through the GPU in bounded
    windows and only the k-mers those queries can look up stay (ipkgpu_db_load_wanted).  The TSV is the same.

    Several -i name a shard set -- ranks' shards, pass files -- whose k-mer sets are disjoint: each file is loaded, the databases are
    united on the GPU (ipkgpu_db_union) and --mu / --omega select from the union; the TSV is that of the merged file.

    --shared-keys: the -i files are branch shards (`build --group-range`), whose k-mer sets may overlap: they are joined in the order
    given (ipkgpu_db_join), the join is filtered with MIF0 and --mu / --omega select from it; the TSV is that of the whole build's file."""
    import ipk_amd
    if shared_keys and stream_db:
        raise click.UsageError("--shared-keys does not go with --stream-db: the join holds every shard on the GPU")
    if len(db_paths) > 1 and stream_db:
        raise click.UsageError("--stream-db takes one -i: a shard set is united on the GPU, which holds every shard")
    db_path = db_paths[0]
    head = None
    if len(db_paths) > 1 or shared_keys:
        head = _shard_set_head(db_paths)
    n_nodes = _join_num_nodes(head, num_tree_nodes) if shared_keys else 0
    for p in db_paths:
        _check_selection(p, mu, omega)
    with open(queries) as fh:
        recs = read_fasta(fh.read())
    eng = ipk_amd.Engine(device)
    try:
        d = None
        if stream_db:
            res = eng.place_file(db_path, [s for _, s in recs], keep_at_most=keep_at_most, ambiguity=expand_ambiguous, strands=strands, mu=mu, omega=omega,
                                 query_batch=query_batch)
        elif shared_keys:
            srcs = []
            try:
                for p in db_paths:
                    srcs.append(eng.load_db(p))
                whole = eng.join_dbs(srcs)
            finally:
                for s in srcs:
                    s.free()
            sigma = {"DNA": 4, "AA": 20}[head["sequence_type"]]
            whole.filter_mif0(eng, n_nodes, ipk_amd.score_threshold(head["omega"], sigma, head["kmer_size"]))
            whole.header = dict(head, total_num_kmers=whole.num_keys, total_num_entries=whole.num_entries)
            d = whole
            if mu is not None or omega is not None:
                d = eng.select_db(whole, mu=mu, omega=omega)
                whole.free()
            res = eng.place(d, [s for _, s in recs], keep_at_most=keep_at_most, ambiguity=expand_ambiguous, strands=strands)
        elif len(db_paths) > 1:
            whole, _ = eng.load_dbs(db_paths)
            d = whole
            if mu is not None or omega is not None:
                d = eng.select_db(whole, mu=mu, omega=omega)
                whole.free()
            res = eng.place(d, [s for _, s in recs], keep_at_most=keep_at_most, ambiguity=expand_ambiguous, strands=strands)
        else:
            d = eng.load_db(db_path, mu=mu, omega=omega)
            res = eng.place(d, [s for _, s in recs], keep_at_most=keep_at_most, ambiguity=expand_ambiguous, strands=strands)
        text = "".join(line + "\n" for line in placement_lines([n for n, _ in recs], res, keep_factor, strands == "both"))
        if output:
            with open(output, "w") as fh:
                fh.write(text)
        else:
            click.echo(text, nl=False)
        if d is not None:
            d.free()
    finally:
        eng.close()


# ---- joining shard files ---------------------------------------------------------------------------------------------------------

def _shard_set_head(paths):
    """The head of a shard set (engine.shard_set_head); a file that disagrees is a usage error that names it."""
    from ipk_amd import dbfile
    from ipk_amd.engine import IpkGpuError, shard_set_head
    try:
        return shard_set_head([dbfile.file_info(p) for p in paths], list(paths))
    except IpkGpuError as e:
        raise click.UsageError(str(e))
    except ValueError as e:
        raise click.UsageError(str(e))


def _join_num_nodes(head, num_tree_nodes):
    """MIF0's N of a join: --num-tree-nodes, else the node count of the shard set's tree index; neither is a usage error."""
    if num_tree_nodes < 0:
        raise click.UsageError("--num-tree-nodes must be positive")
    n = num_tree_nodes or len(head["tree_index"])
    if not n:
        raise click.UsageError("--shared-keys: MIF0 needs the tree's node count and the shards carry no tree index: give --num-tree-nodes")
    return n


@ipk.command()
@click.option("-o", "--output", required=True, help="the merged database file")
@click.option("--on", "on", type=click.Choice(["device", "host"]), default="device", show_default=True,
              help="device: the shards are loaded, united on the GPU and written by the device writer; host: the streaming merge on the host (no GPU)")
@click.option("--shared-keys", is_flag=True, default=False,
              help="the files' k-mer sets may overlap (branch shards of `build --group-range`): a shared k-mer's entries are joined in the "
                   "order of the files, one entry per branch with `put`'s maximum, and the join is filtered anew; --on device only")
@click.option("--filter", "filter_", type=click.Choice(["mif0", "random"]), default="mif0", show_default=True, help="with --shared-keys: the filter of the output")
@click.option("--num-tree-nodes", type=int, default=0, help="with --shared-keys: MIF0's N [the node count of the first shard's tree index]")
@click.option("--stream", is_flag=True, default=False,
              help="with --shared-keys: join by key ranges, no shard ever on the GPU whole: for shards that do not fit device memory together (same output)")
@click.option("--budget-mib", type=float, default=None, help="with --stream: the device memory (MiB) the join may use on top of what the engine holds [what is free]")
@click.option("--tmp-dir", default=None, type=click.Path(file_okay=False), help="with --stream: where the range files live until they are merged [OUTPUT.ranges]")
@click.option("--device", type=int, default=0, show_default=True, help="GPU index")
@click.argument("shards", nargs=-1, required=True, type=click.Path(exists=True, dir_okay=False))
def merge(output, on, shared_keys, filter_, num_tree_nodes, stream, budget_mib, tmp_dir, device, shards):
    """Joins database files with disjoint k-mer sets -- the shards of several ranks, the files of key-range passes, the batches of an
    on-disk build -- into one database file, its records in filter order.

    The shards must agree on sequence type, k, omega and the positions flag.  The tree of the output is that of the first shard
    that carries one (pass files and ranks' shards carry none).  Both routes write the same bytes for shards that are each in filter
    order, as every build writes them.  --on device needs every shard and their union in device memory at once; when they do not fit
    it says so and the host merge takes over.

    --shared-keys joins files whose k-mer sets may overlap, in the order given: branch shards, built over different branch groups of
    one tree (`build --group-range`).  The shards of contiguous group ranges, given in range order and filtered as the build was,
    give the whole build's file byte for byte.  The join needs every shard and the result in device memory; there is no host route.

    --shared-keys --stream is for shards that do not fit: the same file, joined by key ranges that each fit the device (or
    --budget-mib) -- one histogram pass over every shard, then per range the shards' records of that range loaded, joined, filtered and
    written as a range file under --tmp-dir; the host merge makes the output of the range files (ipkgpu_db_join_files)."""
    from ipk_amd import dbfile
    if stream and not shared_keys:
        raise click.UsageError("--stream goes with --shared-keys: shards with disjoint k-mer sets that do not fit are merged on the host (--on host)")
    if (budget_mib is not None or tmp_dir is not None) and not stream:
        raise click.UsageError("--budget-mib and --tmp-dir go with --stream")
    if budget_mib is not None and not budget_mib > 0:
        raise click.UsageError("--budget-mib must be positive")
    head = _shard_set_head(shards)
    if shared_keys:
        if on != "device":
            raise click.UsageError("--shared-keys goes with --on device only: the host merge cannot join the entries of a shared k-mer")
        n_nodes = _join_num_nodes(head, num_tree_nodes) if filter_ == "mif0" else 0
        import ipk_amd
        from ipk_amd.engine import ERR_NOMEM, IpkGpuError
        eng = ipk_amd.Engine(device)
        if stream:
            try:
                if budget_mib is not None:
                    eng.set_option("release_workspaces", 1)
                    eng.set_option("device_budget_bytes", eng.mem_stats()[0] + int(budget_mib * (1 << 20)))
                try:
                    nk, ne, dropped = dbfile.join_shard_files_streamed(eng, output, head["sequence_type"], head["tree_index"], head["newick"], head["kmer_size"],
                                                                       head["omega"], list(shards), filter_, n_nodes, tmp_dir=tmp_dir)
                except IpkGpuError as e:
                    if e.code != ERR_NOMEM:
                        raise
                    click.echo(f"merge: {e}", err=True)
                    sys.exit(1)
                n_ranges = len(eng.join_files_ranges())
            finally:
                eng.close()
            click.echo(f"Output: {output} ({nk} k-mers, {ne} entries; merged on the device; {dropped} entries joined by put; joined in {n_ranges} key ranges)")
            return
        try:
            nk, ne, dropped = dbfile.join_shard_files(eng, output, head["sequence_type"], head["tree_index"], head["newick"], head["kmer_size"],
                                                      head["omega"], list(shards), filter_, n_nodes)
        except IpkGpuError as e:
            if e.code != ERR_NOMEM:
                raise
            click.echo(f"merge: the shards and their join do not fit device memory ({e}); there is no host route for shared k-mers", err=True)
            sys.exit(1)
        finally:
            eng.close()
        click.echo(f"Output: {output} ({nk} k-mers, {ne} entries; merged on the device; {dropped} entries joined by put)")
        return
    if num_tree_nodes or filter_ != "mif0":
        raise click.UsageError("--filter and --num-tree-nodes go with --shared-keys: a merge of disjoint k-mer sets keeps the shards' filter values")
    args = (head["sequence_type"], head["tree_index"], head["newick"], head["kmer_size"], head["omega"], list(shards))
    route = on
    if on == "device":
        import ipk_amd
        from ipk_amd.engine import ERR_NOMEM, IpkGpuError
        eng = ipk_amd.Engine(device)
        try:
            totals = dbfile.union_shard_files(eng, output, *args)
        except IpkGpuError as e:
            if e.code != ERR_NOMEM:
                raise
            click.echo(f"merge: the shards and their union do not fit device memory ({e}); merging on the host", err=True)
            route = "host"
        finally:
            eng.close()
    if route == "host":
        totals = dbfile.merge_shard_files(output, *args)
    click.echo(f"Output: {output} ({totals[0]} k-mers, {totals[1]} entries; merged on the {route})")


if __name__ == "__main__":
    ipk()
