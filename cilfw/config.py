"""CLI / config for cilfw.

Reproduces the reference's flag surface (reference ``template.py:13-49``,
``get_args_parser``) so existing run commands keep working, plus cilfw-native flags for
the MI355X build (dtype, backend selection, checkpoint dir, synthetic data).

Like the reference, the parsed Namespace doubles as the mutable run state: the
orchestrator attaches ``class_order``, ``nb_classes``, ``task_id``, ``known_classes``
and ``increment_per_task`` during the run (reference ``template.py:201-303``).
"""

import argparse


def get_args_parser():
    parser = argparse.ArgumentParser("cilfw class-incremental training", add_help=False)

    # reproducibility (reference default: seed=0, template.py:16)
    parser.add_argument("--seed", default=0, type=int)

    # CIL protocol (reference template.py:16-19)
    parser.add_argument("--num_bases", default=50, type=int,
                        help="classes in the base (first) task")
    parser.add_argument("--increment", default=10, type=int,
                        help="classes added per subsequent task")

    # model / input (reference template.py:20-22)
    parser.add_argument("--backbone", default="resnet32", type=str,
                        choices=["resnet20", "resnet32", "resnet44", "resnet56",
                                 "resnet110", "resnet18", "resnet34", "resnet50"])
    parser.add_argument("--batch_size", default=128, type=int, help="per-GPU batch size")
    parser.add_argument("--input_size", default=32, type=int)

    # augmentation (reference template.py:23-33)
    parser.add_argument("--color_jitter", type=float, default=0.4)
    parser.add_argument("--aa", type=str, default="rand-m9-mstd0.5-inc1",
                        help='RandAugment policy ("" disables)')
    parser.add_argument("--train_interpolation", type=str, default="bicubic")
    parser.add_argument("--reprob", type=float, default=0.0,
                        help="random erasing prob (reference default 0.0)")
    parser.add_argument("--remode", type=str, default="pixel")
    parser.add_argument("--recount", type=int, default=1)
    parser.add_argument("--resplit", action="store_true", default=False)

    # rehearsal memory (reference template.py:34-36)
    parser.add_argument("--herding_method", default="barycenter", type=str,
                        choices=["barycenter", "random"])
    parser.add_argument("--memory_size", default=2000, type=int)
    parser.add_argument("--fixed_memory", action="store_true", default=False)

    # optimization (reference template.py:37-42)
    parser.add_argument("--lr", default=0.1, type=float)
    parser.add_argument("--momentum", default=0.9, type=float)
    parser.add_argument("--weight_decay", default=5e-4, type=float)
    parser.add_argument("--num_epochs", default=140, type=int)
    parser.add_argument("--smooth", default=0.0, type=float, help="label smoothing")
    parser.add_argument("--eval_every_epoch", default=5, type=int)

    # distributed (reference template.py:43-44)
    parser.add_argument("--dist_url", default="env://", type=str)

    # dataset (reference template.py:45-46)
    parser.add_argument("--data_set", default="cifar100", type=str,
                        choices=["cifar100", "imagenet100", "imagenet1000", "cub200",
                                 "synthetic", "synthetic_hard"])
    parser.add_argument("--data_path", default="./data/cifar100", type=str)

    # distillation (reference template.py:47-48)
    parser.add_argument("--lambda_kd", default=0.5, type=float)
    parser.add_argument("--dynamic_lambda_kd", action="store_true", default=False,
                        help="scale lambda_kd by known/(known+new) per task "
                             "(the reference parsed but never used this flag — "
                             "template.py:48; here it is honored)")
    parser.add_argument("--kd_temperature", default=2.0, type=float)
    parser.add_argument("--lambda_pod", default=0.0, type=float,
                        help="weight of PODNet's POD-spatial distillation "
                             "over the backbone's stage outputs against the "
                             "frozen teacher; scaled per task by "
                             "sqrt(known_classes / increment) as in the "
                             "paper (0 = off: no map is requested, no POD "
                             "kernel runs; combine with --lambda_kd 0 for "
                             "POD without logit KD)")
    parser.add_argument("--pod_tap", default="post", choices=["post", "pre"],
                        help="maps POD-spatial pools: post = the stage "
                             "outputs, after their last ReLU, which stays "
                             "fused into the BN kernel; pre = the paper's "
                             "tap before that ReLU: the last block of each "
                             "stage then runs an unfused BN + one add+ReLU "
                             "kernel that also writes the pre-activation, "
                             "in every pass (needs --lambda_pod > 0)")
    parser.add_argument("--lambda_flat", default=0.0, type=float,
                        help="weight of the distillation of the final "
                             "embedding against the frozen teacher, 1 - cos "
                             "per sample (LUCIR's less-forget term, PODNet's "
                             "POD-flat); scaled per task by "
                             "sqrt(known_classes / increment) as in both "
                             "papers (0 = off: no kernel of it runs; with "
                             "--lambda_pod it completes PODNet's "
                             "distillation)")
    parser.add_argument("--head", default="linear",
                        choices=["linear", "cosine"],
                        help="classifier head: the growing linear head, "
                             "bias-corrected after each task by weight "
                             "aligning, or the cosine-normalised head of "
                             "LUCIR / PODNet (logits = sigma * cos(feature, "
                             "class weight); no bias, no weight aligning)")
    parser.add_argument("--cos_scale_init", default=1.0, type=float,
                        help="initial value of the cosine head's trained "
                             "scale sigma (LUCIR starts at 1)")
    parser.add_argument("--lambda_mr", default=0.0, type=float,
                        help="weight of LUCIR's margin-ranking loss: each "
                             "old-class sample's ground-truth cosine must "
                             "beat its --mr_k hardest new-class cosines by "
                             "--mr_margin; a mean over the old samples of "
                             "the batch (under DDP: of each rank's batch, "
                             "the per-rank count); constant weight, no sqrt "
                             "factor; needs --head cosine (0 = off: no "
                             "kernel of it runs; with --lambda_flat, "
                             "--lambda_kd 0 and --imprint this is LUCIR)")
    parser.add_argument("--mr_k", default=2, type=int,
                        help="hard negatives per old sample of the "
                             "margin-ranking loss (1..8, at most the number "
                             "of new classes; LUCIR uses 2)")
    parser.add_argument("--mr_margin", default=0.5, type=float,
                        help="margin of the margin-ranking loss, on the "
                             "cosines (>= 0; LUCIR uses 0.5)")
    parser.add_argument("--imprint", action="store_true", default=False,
                        help="LUCIR's class-mean imprinting: before each "
                             "task after the first, set the new cosine "
                             "head's weight rows to the normalised mean of "
                             "the normalised features of their class, "
                             "scaled to the mean norm of the old rows (one "
                             "extra eval pass over the task set per task; "
                             "needs --head cosine)")
    parser.add_argument("--nb_proxy", default=1, type=int,
                        help="proxies per class of the cosine head (1..16): "
                             "above 1 this is PODNet's local similarity "
                             "classifier, each class's logit the "
                             "softmax-weighted mean of its proxies' cosines "
                             "(PODNet uses 10; needs --head cosine; 1 = the "
                             "single-proxy head, no kernel of the reduce "
                             "runs)")
    parser.add_argument("--proxy_init", default="random",
                        choices=["random", "kmeans"],
                        help="start of each new task's proxies: the head's "
                             "random init, or PODNet's k-means: the K "
                             "proxies of a new class start at the K k-means "
                             "centres of its normalised features, scaled to "
                             "the mean norm of the old rows (one extra eval "
                             "pass over the task set and one kernel launch "
                             "per task; needs --head cosine and --nb_proxy "
                             "> 1; random = no kernel of it runs)")
    parser.add_argument("--kmeans_iters", default=100, type=int,
                        help="most Lloyd iterations of --proxy_init kmeans "
                             "(>= 1; it stops earlier once no assignment "
                             "changes)")
    parser.add_argument("--proxy_gamma", default=1.0, type=float,
                        help="sharpness of the softmax over a class's "
                             "proxies (>= 0; 0 = plain mean; PODNet uses 1; "
                             "needs --head cosine)")
    parser.add_argument("--cls_loss", default="ce", choices=["ce", "nca"],
                        help="classification loss: cross entropy (with "
                             "--lambda_kd logit distillation), or PODNet's "
                             "NCA loss, a margin-softmax whose denominator "
                             "leaves out the ground truth, hinged at 0 "
                             "(needs --head cosine, --lambda_kd 0 and "
                             "--smooth 0; with --nb_proxy 10, --lambda_pod "
                             "and --lambda_flat this is PODNet; from "
                             "--cos_scale_init 1 its margin term drives "
                             "sigma below 0, see profiles/lsc_nca.md)")
    parser.add_argument("--nca_margin", default=0.6, type=float,
                        help="margin of the NCA loss, on the cosines (>= 0; "
                             "PODNet uses 0.6)")

    # ---- cilfw-native flags (no reference counterpart) ----
    parser.add_argument("--class_order", default=None, type=str,
                        help="comma-separated class permutation; default: the "
                             "reference's hardcoded CIFAR-100 order "
                             "(template.py:201-202) for cifar100, else a "
                             "seeded permutation")
    parser.add_argument("--dtype", default="bf16", type=str, choices=["bf16", "fp32"],
                        help="compute dtype for the backbone")
    parser.add_argument("--device", default=None, type=str,
                        help="cuda|cpu (default: cuda if available)")
    parser.add_argument("--workers", default=4, type=int)
    parser.add_argument("--output_dir", default="", type=str,
                        help="checkpoint directory ('' disables checkpointing)")
    parser.add_argument("--resume", default="", type=str,
                        help="resume from a per-task checkpoint file")
    parser.add_argument("--synthetic_classes", default=100, type=int,
                        help="class count for --data_set synthetic")
    parser.add_argument("--synthetic_train_size", default=5000, type=int,
                        help="samples per class split across classes for --data_set "
                             "synthetic")
    parser.add_argument("--no_aug", action="store_true", default=False)
    parser.add_argument("--ddp_bucket_mb", default=25.0, type=float,
                        help="gradient all-reduce bucket size (MB)")
    parser.add_argument("--gpu_data", action="store_true", default=False,
                        help="HBM-resident task data + on-device batch "
                             "assembly (crop/flip/normalize) — bypasses the "
                             "Python DataLoader for array-backed datasets "
                             "and, at --input_size > 64, for ImageFolder "
                             "trees (decoded once into a device-resident "
                             "ragged store; CILFW_GPU_DATA_PATHS=0 keeps "
                             "those on the host DataLoader)")
    parser.add_argument("--no_wa", action="store_true", default=False,
                        help="ablation: skip the weight-align step")
    parser.add_argument("--no_replay", action="store_true", default=False,
                        help="ablation: no rehearsal exemplars (forgetting "
                             "baseline)")
    parser.add_argument("--no_device_replay", action="store_true", default=False,
                        help="with --gpu_data, source replay via host "
                             "add_samples instead of the HBM-resident "
                             "DeviceReplayMirror")
    parser.add_argument("--nme_eval", action="store_true", default=False,
                        help="after each task also evaluate with iCaRL's "
                             "nearest-mean-of-exemplars classifier over the "
                             "rehearsal memory (prints NME Acc@1/Acc@5 next "
                             "to the linear head's; training is unchanged)")
    parser.add_argument("--max_tasks", default=0, type=int,
                        help="stop after N tasks (0 = all) — e.g. the "
                             "BASELINE config[0] 2-task plumbing oracle")
    parser.add_argument("--metric_every", default=1, type=int,
                        help="read train metrics to host every N steps "
                             "(1 = reference-exact; higher avoids per-step "
                             "GPU syncs in the hot loop)")
    parser.add_argument("--no_step_graph", action="store_true", default=False,
                        help="disable hipGraph capture of the training step "
                             "(graphs are on by default with --gpu_data)")
    parser.add_argument("--dist_timeout", default=300.0, type=float,
                        help="collective timeout in seconds — a dead rank "
                             "raises instead of hanging (reference behavior "
                             "is an indefinite hang); also drives the "
                             "heartbeat watchdog")
    parser.add_argument("--compat_step_barrier", action="store_true", default=False,
                        help="reproduce the reference's per-training-step "
                             "dist.barrier (template.py:272) — a perf bug kept "
                             "behind a flag")
    return parser


def check_args(args):
    """Flag combinations refused at start-up (ValueError). Also called by
    ``engine.run`` for a Namespace built without ``parse_args``."""
    head = getattr(args, "head", "linear")
    if getattr(args, "lambda_mr", 0.0) > 0 and head != "cosine":
        raise ValueError(
            f"--lambda_mr {args.lambda_mr} needs --head cosine (got --head "
            f"{head}): the margin-ranking loss is defined on cosine logits")
    if getattr(args, "imprint", False) and head != "cosine":
        raise ValueError(
            f"--imprint needs --head cosine (got --head {head}): only a "
            f"cosine head's rows can be set to class means")
    if getattr(args, "lambda_mr", 0.0) > 0:
        if not 1 <= getattr(args, "mr_k", 2) <= 8:
            raise ValueError(f"--mr_k must be in 1..8 (got {args.mr_k})")
        if not getattr(args, "mr_margin", 0.5) >= 0:
            raise ValueError(
                f"--mr_margin must be >= 0 (got {args.mr_margin})")
    if getattr(args, "pod_tap", "post") == "pre" \
            and not getattr(args, "lambda_pod", 0.0) > 0:
        raise ValueError(
            "--pod_tap pre needs --lambda_pod > 0: without POD-spatial "
            "nothing reads the pre-ReLU maps and the unfused block tails "
            "only cost time")
    nb_proxy = getattr(args, "nb_proxy", 1)
    gamma = getattr(args, "proxy_gamma", 1.0)
    if not 1 <= nb_proxy <= 16:
        raise ValueError(f"--nb_proxy must be in 1..16 (got {nb_proxy})")
    if not gamma >= 0:
        raise ValueError(f"--proxy_gamma must be >= 0 (got {gamma})")
    if nb_proxy != 1 and head != "cosine":
        raise ValueError(
            f"--nb_proxy {nb_proxy} needs --head cosine (got --head {head}): "
            f"the proxies are rows of a cosine head")
    if gamma != 1.0 and head != "cosine":
        raise ValueError(
            f"--proxy_gamma {gamma} needs --head cosine (got --head {head}): "
            f"it weights the proxies of a cosine head")
    if getattr(args, "imprint", False) and nb_proxy > 1:
        raise ValueError(
            f"--imprint cannot be combined with --nb_proxy {nb_proxy}: "
            f"identical proxies would never separate")
    if getattr(args, "proxy_init", "random") == "kmeans":
        if head != "cosine":
            raise ValueError(
                f"--proxy_init kmeans needs --head cosine (got --head "
                f"{head}): the proxies are rows of a cosine head")
        if nb_proxy == 1:
            raise ValueError(
                "--proxy_init kmeans needs --nb_proxy > 1: a single proxy "
                "per class is set to the class mean with --imprint")
        if not getattr(args, "kmeans_iters", 100) >= 1:
            raise ValueError(
                f"--kmeans_iters must be >= 1 (got {args.kmeans_iters})")
    if getattr(args, "cls_loss", "ce") == "nca":
        if head != "cosine":
            raise ValueError(
                f"--cls_loss nca needs --head cosine (got --head {head}): "
                f"the NCA loss is defined on cosine logits")
        if getattr(args, "lambda_kd", 0.0) != 0:
            raise ValueError(
                f"--cls_loss nca needs --lambda_kd 0 (got --lambda_kd "
                f"{args.lambda_kd}): logit distillation is fused with the "
                f"cross entropy")
        if getattr(args, "dynamic_lambda_kd", False):
            raise ValueError(
                "--cls_loss nca cannot be combined with --dynamic_lambda_kd: "
                "there is no logit distillation to weight")
        if getattr(args, "smooth", 0.0) != 0:
            raise ValueError(
                f"--cls_loss nca needs --smooth 0 (got --smooth "
                f"{args.smooth}): label smoothing belongs to the cross "
                f"entropy")
        if not getattr(args, "nca_margin", 0.6) >= 0:
            raise ValueError(
                f"--nca_margin must be >= 0 (got {args.nca_margin})")


def parse_args(argv=None):
    parser = argparse.ArgumentParser("cilfw", parents=[get_args_parser()])
    args = parser.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        parser.error(str(e))
    return args
