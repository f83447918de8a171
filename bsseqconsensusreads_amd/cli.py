"""Command lines for the Snakemake rules this package replaces.

    python -m bsseqconsensusreads_amd.cli step5 --reference FA IN.bam OUT.bam [--fastq1 F1 --fastq2 F2]
        rules convert_Bstrain, extend, groupsort_convert, callduplex (main.snake.py:121-164), and
        with --fastq1/--fastq2 also consensusduplex_to_fq (main.snake.py:167-177)
    python -m bsseqconsensusreads_amd.cli molecular IN.bam OUT.bam [--fastq1 F1 --fastq2 F2]
        rule call_consensus_reads_molecular (main.snake.py:46-55) [+ consensus_to_fq_unfiltered]

Both take fgbio FilterConsensusReads' options as --filter-* (DESIGN.md 3.8): with
--filter-min-base-quality the consensus is filtered on the GPU before any output is built, so
OUT.bam and the FASTQ pair hold the kept, masked templates (rule consensus_to_fq's input,
main.snake.py:70-80, with no FilterConsensusReads run; --gpus 1 only).

step5 --groupsort-bam PATH also writes the records after tool 1 and tool 2 in TemplateCoordinate
order: the file rule groupsort_convert leaves (main.snake.py:144-153), the input of fgbio
CallDuplexConsensusReads at :163 (--gpus 1 only).

    python -m bsseqconsensusreads_amd.cli group IN.bam OUT.bam [--edits E] [--min-map-q Q] [--info PATH]
    python -m bsseqconsensusreads_amd.cli zipper ALIGNED.bam UNMAPPED.bam OUT.bam [--tags-to-reverse T..]
            [--tags-to-revcomp T..] [--tags-to-remove T..] [--info PATH] [--stream true --chunk-mb M --tmp-dir DIR]
        rules mergeAunA_consensus and mergeAunA_consensus_grepaligned (main.snake.py:97-119): the aligner's
        records with MI, RX, RG and the consensus tags put back from the step-1 BAM, unmapped records
        dropped, coordinate-sorted on the GPU.  --stream true: memory bounded by
        --chunk-mb (default 1024) -- sorted runs under --tmp-dir, merged on the GPU; ALIGNED must keep
        UNMAPPED's template order, as bwa mem leaves it.  --stream false (the default) reads both inputs whole.

OUT.bam may be '-' to skip the BAM when only the FASTQ pair is wanted.  Errors exit non-zero with
the message on stderr, so Snakemake aborts the rule and removes partial outputs, as it does for
the reference tools (tools/2.extend_gap.py:179-180 raises on a record without MI).

step5 on one GPU streams a coordinate-sorted input (--stream auto, the default: when the header
says SO:coordinate): bounded memory whatever the input size, decode / GPU / encode overlapped,
output identical to the whole-file path (bam.step5_stream).  Other inputs are read whole
(bam.step5); --stream true insists on streaming (an unsorted input is then an error).
step5 --gpus N on a coordinate-sorted input streams too.  --multi ranks (the default;
ranks.step5_ranks): N spawned rank processes (one per GPU) each decode, compute and encode their
own key interval of the file, and this process concatenates their fragments -- no front end.
Mates on other contigs and unmapped mates are spilled and formed in a second phase.  When a
record's owner could not read it (an insert longer than the window slack) the ranks stop and the
file runs as --multi fleet (fleet.step5_stream_multi): this process reads the BAM once
and writes the outputs in order, N spawned worker processes run the family batches it deals them
through shared memory.  Both: bounded memory, output identical to --gpus 1.  Other inputs (or a run under torch.distributed.run) take the whole-file path: one
process per GPU, every rank forms the plan, batches dealt to the ranks, rank 0 writes
(bam.consensus_sharded).  --devices maps workers / ranks to device ids (default 0..N-1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def parse(argv):
    ap = argparse.ArgumentParser(prog="bsseqconsensusreads_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("step5", "molecular"):
        p = sub.add_parser(name)
        if name == "step5":
            p.add_argument("--reference", "-r", required=True, help="FASTA of the alignment (tools/1 --reference)")
        p.add_argument("input")
        p.add_argument("output", help="consensus BAM, or '-' for none")
        p.add_argument("--fastq1")
        p.add_argument("--fastq2")
        p.add_argument("--read-name-prefix", default=None)
        p.add_argument("--threads", type=int, default=8)
        p.add_argument("--compression", type=int, default=6)
        p.add_argument("--device", type=int, default=0)
        p.add_argument("--gpu-bgzf", default="false", choices=("true", "false"),
                       help="deflate the output BAM's and FASTQ pair's blocks on the GPU (streaming; files ~4%% larger)")
        p.add_argument("--gpu-inflate", default="false", choices=("true", "false"),
                       help="inflate the input BAM's BGZF blocks on the GPU (streaming, --gpus 1; the same output)")
        p.add_argument("--gpu-fastq", default="false", choices=("true", "false"),
                       help="format, checksum and deflate the FASTQ pair on the GPU (streaming, --gpus 1; needs "
                            "--fastq1/--fastq2; the files of a --gpu-bgzf run)")
        p.add_argument("--gpu-bam", default="false", choices=("true", "false"),
                       help="write, checksum and deflate the output BAM's records (consensus tags included) on the "
                            "GPU (streaming, --gpus 1; needs OUT.bam; implies the GPU deflate for the BAM; the file "
                            "of a --gpu-bgzf run)")
        p.add_argument("--gpu-image", default="false", choices=("true", "false"),
                       help="make the family images on the GPU from the records' SEQ / QUAL bytes instead of "
                            "unpacking and copying every base on the host (streaming, --gpus 1; the same output "
                            "files)")
        p.add_argument("--metrics", default=None, metavar="PATH",
                       help="write the run's consensus metrics, reduced on the GPU, as one JSON file: histograms of "
                            "cD/aD/bD and cE/aE/bE per record, of the consensus quality, and per-cycle depth, errors, "
                            "quality, no-calls and strand disagreements of the unfiltered consensus (--gpus 1; the "
                            "same output files)")
        p.add_argument("--metrics-cycles", type=int, default=512, metavar="N",
                       help="rows of the per-cycle table, 2..1024; columns at and past N - 1 share the last row")
        # (registered for both commands: molecular refuses it with the reason, below)
        p.add_argument("--groupsort-bam", default=None, metavar="PATH",
                       help="also write the records after tool 1 and tool 2, in fgbio TemplateCoordinate order, as "
                            "the BAM rule groupsort_convert leaves (the input of fgbio CallDuplexConsensusReads): "
                            "encoded on the GPU from the stage dump, unfiltered whatever --filter-* says (--gpus 1; "
                            "the same output files)")
        p.add_argument("--batch-bases", type=int, default=None, help="device batch budget in bases")
        p.add_argument("--chunk-mb", type=int, default=64, help="--stream: record MiB per chunk")
        if name == "step5":
            p.add_argument("--gpus", type=int, default=1, help="one process per GPU, family batches dealt to them")
            p.add_argument("--devices", default=None, help="comma-separated device id per rank (default 0..gpus-1)")
            p.add_argument("--multi", default="ranks", choices=["ranks", "fleet"],
                           help="--gpus N on a coordinate-sorted input: ranks = each GPU's process reads, computes "
                                "and writes its own part of the file (ranks.py; fleet when a record's owner could "
                                "not read it); fleet = one process reads and writes, the GPUs' processes compute")
            p.add_argument("--stream", default="auto", choices=["auto", "true", "false"],
                           help="bounded-memory pipelined step (bam.step5_stream; coordinate-sorted input); "
                                "false = read the whole BAM first (bam.step5); auto = stream when the header "
                                "says SO:coordinate")
        else:
            p.add_argument("--min-consensus-base-quality", type=int, default=0,
                           help="mask single-strand calls below this phred to N (main.snake.py:54 passes 0)")
            p.add_argument("--stream", default="true", choices=["true", "false"],
                           help="bounded-memory pipelined step cut between MI runs (bam.molecular_stream; the "
                                "GroupReadsByUmi order of the input); false = read the whole BAM first")
        p.add_argument("--output-per-base-tags", default="true", choices=["true", "false"],
                       help="fgbio's consensus tags (per-read and per-base statistics); off = name/SEQ/QUAL/RG/MI/RX")
        g = p.add_argument_group("consensus filter (fgbio FilterConsensusReads; off unless --filter-min-base-quality)")
        g.add_argument("--filter-min-base-quality", type=int, default=None, metavar="Q",
                       help="-N: mask consensus bases below Q to N; turns the filter on")
        g.add_argument("--filter-min-reads", type=int, nargs="+", default=None, metavar="M",
                       help="-M: one to three values, duplex / AB / BA (default 1)")
        g.add_argument("--filter-max-read-error-rate", type=float, nargs="+", default=None, metavar="E",
                       help="-E: one to three values (default 0.025)")
        g.add_argument("--filter-max-base-error-rate", type=float, nargs="+", default=None, metavar="E",
                       help="-e: one to three values (default 0.1)")
        g.add_argument("--filter-max-no-call-fraction", type=float, default=None, metavar="F", help="-n (default 0.2)")
        g.add_argument("--filter-min-mean-base-quality", type=int, default=None, metavar="Q", help="-q (default: off)")
        g.add_argument("--filter-require-single-strand-agreement", default=None, choices=("true", "false"),
                       help="-s: mask duplex bases whose two single-strand calls differ (default false)")
    z = sub.add_parser("zipper")
    z.add_argument("aligned", help="the aligner's BAM of the step-1 FASTQ pair (any order)")
    z.add_argument("unmapped", help="the step-1 consensus BAM (unmapped records with MI, RX, RG and the consensus tags)")
    z.add_argument("output", help="the coordinate-sorted, mapped-only BAM with the tags put back (step5's input)")
    for opt, what in (("reverse", "reversed"), ("revcomp", "reverse-complemented")):
        z.add_argument("--tags-to-" + opt, nargs="*", default=[], metavar="T",
                       help="tags of the unmapped record that are %s on a reverse-strand record; Consensus = fgbio's "
                            "per-base consensus tags (default: none, as main.snake.py:106)" % what)
    z.add_argument("--tags-to-remove", nargs="*", default=[], metavar="T", help="tags left out of the output records")
    z.add_argument("--threads", type=int, default=8)
    z.add_argument("--level", type=int, default=6, help="the output's deflate level")
    z.add_argument("--device", type=int, default=0)
    z.add_argument("--info", default=None, metavar="PATH", help="write the run's counts as one JSON file")
    z.add_argument("--stream", default="false", choices=("true", "false"),
                   help="bounded memory: sorted runs of --chunk-mb each, merged on the GPU; needs ALIGNED to keep "
                        "UNMAPPED's template order, as bwa mem leaves it (default false: both inputs are read whole)")
    z.add_argument("--chunk-mb", type=int, default=1024, metavar="M",
                   help="--stream true: the MiB of record bytes (ALIGNED's records and their partners' tags) a run holds")
    z.add_argument("--tmp-dir", default=None, metavar="DIR", help="--stream true: where the runs are kept (default: OUT's directory)")
    g = sub.add_parser("group")
    g.add_argument("input", help="the aligned, UMI-tagged BAM (any order; read whole)")
    g.add_argument("output", help="the grouped BAM (cli molecular's input)")
    g.add_argument("--strategy", default="paired", help="only 'paired' is built")
    g.add_argument("--edits", type=int, default=1, help="the most differing UMI bases that still join (0..3)")
    g.add_argument("--min-map-q", type=int, default=1)
    g.add_argument("--include-non-pf-reads", default="false", choices=("true", "false"))
    g.add_argument("--raw-tag", default="RX")
    g.add_argument("--assign-tag", default="MI")
    g.add_argument("--threads", type=int, default=8)
    g.add_argument("--level", type=int, default=6, help="the output's deflate level")
    g.add_argument("--device", type=int, default=0)
    g.add_argument("--info", default=None, metavar="PATH", help="write the run's counts as one JSON file")
    a = ap.parse_args(argv)
    if a.cmd == "group":
        if a.strategy.lower() != "paired":
            ap.error("--strategy %s is not built: only 'paired' is" % a.strategy)
        if not 0 <= a.edits <= 3:
            ap.error("--edits takes 0..3")
        return a
    if a.cmd == "zipper":
        if a.chunk_mb < 1:
            ap.error("--chunk-mb takes a positive number")
        return a
    others = [k for k in ("min_reads", "max_read_error_rate", "max_base_error_rate", "max_no_call_fraction",
                          "min_mean_base_quality", "require_single_strand_agreement")
              if getattr(a, "filter_" + k) is not None]
    if a.filter_min_base_quality is None and others:
        ap.error("--filter-%s needs --filter-min-base-quality (which turns the filter on)" % others[0].replace("_", "-"))
    for k in ("min_reads", "max_read_error_rate", "max_base_error_rate"):
        if getattr(a, "filter_" + k) is not None and len(getattr(a, "filter_" + k)) > 3:
            ap.error("--filter-%s takes one to three values" % k.replace("_", "-"))
    if a.filter_min_base_quality is not None and getattr(a, "gpus", 1) > 1:
        ap.error("the consensus filter is not supported with --gpus %d yet" % a.gpus)
    if (a.fastq1 is None) != (a.fastq2 is None):
        ap.error("--fastq1 and --fastq2 go together")
    if a.output == "-" and a.fastq1 is None:
        ap.error("nothing to write: give OUT.bam or --fastq1/--fastq2")
    if a.groupsort_bam is not None and a.cmd != "step5":
        ap.error("--groupsort-bam applies to step5 only: %s (step 1) runs no tools, so there are no tool-stage "
                 "records to write" % a.cmd)
    if a.groupsort_bam is not None and a.gpus > 1:
        ap.error("--groupsort-bam is not supported with --gpus %d yet (one process, one GPU)" % a.gpus)
    if a.metrics is not None and getattr(a, "gpus", 1) > 1:
        ap.error("--metrics is not supported with --gpus %d yet (one process, one GPU)" % a.gpus)
    if not 2 <= a.metrics_cycles <= 1024:
        ap.error("--metrics-cycles takes 2..1024")
    if a.gpu_inflate == "true" and getattr(a, "gpus", 1) > 1:
        ap.error("--gpu-inflate is not supported with --gpus %d yet (the rank processes start without torch)" % a.gpus)
    if a.gpu_fastq == "true":
        if a.fastq1 is None:
            ap.error("--gpu-fastq needs --fastq1/--fastq2")
        if getattr(a, "gpus", 1) > 1:
            ap.error("--gpu-fastq is not supported with --gpus %d yet (one process, one GPU)" % a.gpus)
        if a.stream == "false":
            ap.error("--gpu-fastq applies to the streaming step only: not with --stream false")
    if a.gpu_bam == "true":
        if a.output == "-":
            ap.error("--gpu-bam needs the output BAM: not with OUT.bam '-'")
        if getattr(a, "gpus", 1) > 1:
            ap.error("--gpu-bam is not supported with --gpus %d yet (one process, one GPU)" % a.gpus)
        if a.stream == "false":
            ap.error("--gpu-bam applies to the streaming step only: not with --stream false")
    if a.gpu_image == "true":
        if getattr(a, "gpus", 1) > 1:
            ap.error("--gpu-image is not supported with --gpus %d yet (one process, one GPU)" % a.gpus)
        if a.stream == "false":
            ap.error("--gpu-image applies to the streaming step only: not with --stream false")
    if a.gpu_inflate == "true" and a.stream == "false":
        print("warning: --gpu-inflate applies to the streaming step only; --stream false inflates on the host",
              file=sys.stderr)
    if a.gpu_bgzf == "true" and a.stream == "false":
        print("warning: --gpu-bgzf applies to the streaming step only; --stream false deflates on the host",
              file=sys.stderr)
    return a


def filter_params(a):
    """The --filter-* options as filter.FilterParams, None when the filter is off."""
    if a.filter_min_base_quality is None:
        return None
    from .filter import FilterParams
    kw = {k: getattr(a, "filter_" + k) for k in ("max_no_call_fraction", "min_mean_base_quality")}
    kw.update({k: tuple(getattr(a, "filter_" + k)) for k in ("min_reads", "max_read_error_rate", "max_base_error_rate")
               if getattr(a, "filter_" + k) is not None})
    kw["require_single_strand_agreement"] = a.filter_require_single_strand_agreement == "true"
    return FilterParams(a.filter_min_base_quality, **{k: v for k, v in kw.items() if v is not None})


def _coordinate_sorted(bam, path: str) -> bool:
    """The header's @HD SO tag says coordinate (what the streaming reader needs)."""
    for line in bam.read_bam_header(path).text.splitlines():
        if line.startswith("@HD"):
            return "\tSO:coordinate" in "\t" + line.split("\t", 1)[-1]
    return False


def _step5_fleet(a, gpus: int) -> int:
    """step5 --gpus N on a coordinate-sorted input: ranks.step5_ranks, or fleet.step5_stream_multi
    (module docstring)."""
    from . import ranks  # (fleet, with torch, only if it runs)
    devs = [int(x) for x in a.devices.split(",")] if a.devices else list(range(gpus))
    if len(devs) != gpus:
        print("--devices needs %d ids" % gpus, file=sys.stderr)
        return 2
    if a.multi == "ranks":
        try:
            info = ranks.step5_ranks(a.input, a.reference, None if a.output == "-" else a.output, devs,
                                     a.read_name_prefix, a.threads, a.compression,
                                     (a.fastq1, a.fastq2) if a.fastq1 else None,
                                     tags=a.output_per_base_tags == "true", chunk_bytes=a.chunk_mb << 20,
                                     batch_bases=a.batch_bases, gpu_bgzf=a.gpu_bgzf == "true", on_foreign="raise")
            print(json.dumps(info), file=sys.stderr)
            return 0
        except ranks.ForeignRecords as e:
            print("ranks: %s; running --multi fleet" % e, file=sys.stderr)
        except Exception as e:  # noqa: BLE001 -- the rule fails with the message
            print("%s: %s" % (type(e).__name__, e), file=sys.stderr)
            return 1
    from . import fleet
    try:
        info = fleet.step5_stream_multi(a.input, a.reference, None if a.output == "-" else a.output, devs,
                                        a.read_name_prefix, a.threads, a.compression,
                                        (a.fastq1, a.fastq2) if a.fastq1 else None,
                                        tags=a.output_per_base_tags == "true", chunk_bytes=a.chunk_mb << 20,
                                        batch_bases=a.batch_bases, gpu_bgzf=a.gpu_bgzf == "true")
    except Exception as e:  # noqa: BLE001 -- the rule fails with the message
        print("%s: %s" % (type(e).__name__, e), file=sys.stderr)
        return 1
    print(json.dumps(info), file=sys.stderr)
    return 0


def _zipper(a) -> int:
    """cli zipper: rules mergeAunA_consensus + mergeAunA_consensus_grepaligned on one GPU (zipper.zipper)."""
    try:
        from . import bam
        info = bam.zipper(a.aligned, a.unmapped, a.output, a.tags_to_reverse, a.tags_to_revcomp, a.tags_to_remove,
                          threads=a.threads, level=a.level, device=a.device, info=a.info, stream=a.stream == "true",
                          chunk_bytes=a.chunk_mb << 20, tmp_dir=a.tmp_dir)
    except Exception as e:  # noqa: BLE001 -- the rule fails with the message
        print("%s: %s" % (type(e).__name__, e), file=sys.stderr)
        return 1
    print(json.dumps(info), file=sys.stderr)
    return 0


def _group(a) -> int:
    """cli group: fgbio GroupReadsByUmi -s Paired on one GPU (group.group)."""
    try:
        from . import bam
        info = bam.group(a.input, a.output, a.edits, a.min_map_q, a.include_non_pf_reads == "true", a.raw_tag,
                         a.assign_tag, a.strategy, threads=a.threads, level=a.level, device=a.device, info=a.info)
    except Exception as e:  # noqa: BLE001 -- the rule fails with the message
        print("%s: %s" % (type(e).__name__, e), file=sys.stderr)
        return 1
    print(json.dumps(info), file=sys.stderr)
    return 0


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parse(argv)
    if a.cmd == "group":
        return _group(a)
    if a.cmd == "zipper":
        return _zipper(a)
    from . import bam, shard
    gpus = getattr(a, "gpus", 1)
    if gpus > 1 and "WORLD_SIZE" not in os.environ:
        if a.stream == "true" or (a.stream == "auto" and _coordinate_sorted(bam, a.input)):
            return _step5_fleet(a, gpus)  # this process never touches the GPU
        return shard.launch(gpus, main, (argv,))  # this process never touches the GPU
    rank, world, local = shard.env_rank()
    if world != gpus:
        print("--gpus %d but WORLD_SIZE=%d" % (gpus, world), file=sys.stderr)
        return 2
    device = a.device
    if world > 1:
        devs = [int(x) for x in a.devices.split(",")] if a.devices else list(range(world))
        if len(devs) != world:
            print("--devices needs %d ids" % world, file=sys.stderr)
            return 2
        device = devs[local]
    from .device import Engine
    out = None if a.output == "-" else a.output
    fq = (a.fastq1, a.fastq2) if a.fastq1 else None
    flt = filter_params(a)
    dist = None
    try:
        dist = shard.init("gloo") if world > 1 else None  # host gather of the batch outputs only
        eng = Engine(device)
        try:
            stream = a.cmd == "step5" and world == 1 and (
                a.stream == "true" or (a.stream == "auto" and _coordinate_sorted(bam, a.input)))
            if stream:
                info = bam.step5_stream(a.input, a.reference, out, eng, a.read_name_prefix, a.threads, a.compression,
                                        fq, tags=a.output_per_base_tags == "true", chunk_bytes=a.chunk_mb << 20,
                                        batch_bases=a.batch_bases, gpu_bgzf=a.gpu_bgzf == "true", filter=flt,
                                        gpu_inflate=a.gpu_inflate == "true", gpu_fastq=a.gpu_fastq == "true",
                                        gpu_bam=a.gpu_bam == "true", gpu_image=a.gpu_image == "true",
                                        metrics=a.metrics, metrics_cycles=a.metrics_cycles,
                                        **({"groupsort_bam": a.groupsort_bam} if a.groupsort_bam else {}))
            elif a.cmd == "step5" and a.gpu_image == "true":
                raise ValueError("--gpu-image applies to the streaming step only: %s is not coordinate-sorted "
                                 "and would be read whole" % a.input)
            elif a.cmd == "step5" and a.gpu_bam == "true":
                raise ValueError("--gpu-bam applies to the streaming step only: %s is not coordinate-sorted "
                                 "and would be read whole" % a.input)
            elif a.cmd == "step5" and a.gpu_fastq == "true":
                raise ValueError("--gpu-fastq applies to the streaming step only: %s is not coordinate-sorted "
                                 "and would be read whole" % a.input)
            elif a.cmd == "step5":
                info = bam.step5(a.input, a.reference, out, eng, a.read_name_prefix, a.threads, a.compression, fq,
                                 tags=a.output_per_base_tags == "true", batch_bases=a.batch_bases, dist=dist,
                                 filter=flt, metrics=a.metrics, metrics_cycles=a.metrics_cycles,
                                 **({"groupsort_bam": a.groupsort_bam} if a.groupsort_bam else {}))
            elif a.stream == "true":
                info = bam.molecular_stream(a.input, out, eng, a.read_name_prefix, a.threads, a.compression, fq,
                                            tags=a.output_per_base_tags == "true", chunk_bytes=a.chunk_mb << 20,
                                            batch_bases=a.batch_bases, gpu_bgzf=a.gpu_bgzf == "true",
                                            min_consensus_base_quality=a.min_consensus_base_quality, filter=flt,
                                            gpu_inflate=a.gpu_inflate == "true", gpu_fastq=a.gpu_fastq == "true",
                                            gpu_bam=a.gpu_bam == "true", gpu_image=a.gpu_image == "true",
                                            metrics=a.metrics, metrics_cycles=a.metrics_cycles)
            else:
                info = bam.molecular(a.input, out, eng, a.read_name_prefix, a.threads, a.compression, fq,
                                     tags=a.output_per_base_tags == "true",
                                     min_consensus_base_quality=a.min_consensus_base_quality, filter=flt,
                                     metrics=a.metrics, metrics_cycles=a.metrics_cycles)
        finally:
            eng.close()
    except Exception as e:  # noqa: BLE001 -- the rule fails with the message, like the tools do
        print("%s: %s" % (type(e).__name__, e), file=sys.stderr)
        return 1
    finally:
        if dist is not None:
            dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(info), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
