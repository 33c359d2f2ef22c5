"""Command-line options: every flag of the reference's ``MonodepthOptions`` (MD2/options.py:15-233) keeps
its spelling, type and default.  Added (marked NEW): the attack hyper-parameters that the reference
hard-codes in MD2/trainer.py:199-223, a synthetic dataset, and the data-parallel switches."""
import argparse
import os

file_dir = os.path.dirname(__file__)


class MonodepthOptions:
    def __init__(self):
        p = argparse.ArgumentParser(description="Monodepthv2 options (MI355X adversarial-training build)")
        # PATHS
        p.add_argument("--data_path", type=str, default=os.path.join(file_dir, "kitti_data"))
        p.add_argument("--log_dir", type=str, default=os.path.join(os.path.expanduser("~"), "tmp"))
        # TRAINING
        p.add_argument("--model_name", type=str, default="mdp")
        p.add_argument("--split", type=str, choices=["eigen_zhou", "eigen_full", "odom", "benchmark"],
                       default="eigen_zhou")
        p.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152])
        p.add_argument("--dataset", type=str, default="kitti",
                       choices=["kitti", "kitti_odom", "kitti_depth", "kitti_test", "synthetic"])
        p.add_argument("--png", action="store_true")
        p.add_argument("--height", type=int, default=192)
        p.add_argument("--width", type=int, default=640)
        p.add_argument("--disparity_smoothness", type=float, default=1e-3)
        p.add_argument("--scales", nargs="+", type=int, default=[0, 1, 2, 3])
        p.add_argument("--min_depth", type=float, default=0.1)
        p.add_argument("--max_depth", type=float, default=100.0)
        p.add_argument("--use_stereo", action="store_true")
        p.add_argument("--frame_ids", nargs="+", type=int, default=[0, -1, 1])
        p.add_argument("--adv_train", action="store_true", help="do adversarial training")
        p.add_argument("--fine_tune", action="store_true", help="do finetune on an existing model")
        p.add_argument("--supervised_adv", action="store_true", help="add the supervised loss on the adversarial view")
        # no default, as in the reference (MD2/options.py:94-96); Trainer.__init__ asks for it under --adv_train, where the
        # reference would run into a NameError at MD2/trainer.py:224 (neither branch assigns ``args``)
        p.add_argument("--norm_type", type=str, choices=["l_inf", "l_0"])
        # OPTIMIZATION
        p.add_argument("--batch_size", type=int, default=12)
        p.add_argument("--learning_rate", type=float, default=1e-4)
        p.add_argument("--num_epochs", type=int, default=20)
        p.add_argument("--scheduler_step_size", type=int, default=15)
        # ABLATION
        p.add_argument("--v1_multiscale", action="store_true")
        p.add_argument("--avg_reprojection", action="store_true")
        p.add_argument("--disable_automasking", action="store_true")
        p.add_argument("--predictive_mask", action="store_true")
        p.add_argument("--no_ssim", action="store_true")
        p.add_argument("--weights_init", type=str, default="pretrained", choices=["pretrained", "scratch"])
        p.add_argument("--pose_model_input", type=str, default="pairs", choices=["pairs", "all"])
        p.add_argument("--pose_model_type", type=str, default="separate_resnet",
                       choices=["posecnn", "separate_resnet", "shared"])
        p.add_argument("--contrastive_learning", action="store_true")
        p.add_argument("--no_original_train", action="store_true")
        p.add_argument("--half_no_synthesis", action="store_true")
        # SYSTEM
        p.add_argument("--no_cuda", action="store_true")
        p.add_argument("--num_workers", type=int, default=12)
        # LOADING
        p.add_argument("--load_weights_folder", type=str)
        p.add_argument("--models_to_load", nargs="+", type=str, default=["encoder", "depth", "pose_encoder", "pose"])
        # LOGGING
        p.add_argument("--log_frequency", type=int, default=250)
        p.add_argument("--save_frequency", type=int, default=1)
        # EVALUATION (read by evaluate_depth.evaluate; --eval_split odom_9 / odom_10 by evaluate_pose.evaluate; --eval_out_dir
        # belongs to the benchmark export, which is out of scope)
        p.add_argument("--eval_stereo", action="store_true")
        p.add_argument("--eval_mono", action="store_true")
        p.add_argument("--disable_median_scaling", action="store_true")
        p.add_argument("--pred_depth_scale_factor", type=float, default=1)
        p.add_argument("--ext_disp_to_eval", type=str)
        p.add_argument("--eval_split", type=str, default="eigen",
                       choices=["eigen", "eigen_benchmark", "benchmark", "odom_9", "odom_10"])
        p.add_argument("--save_pred_disps", action="store_true")
        p.add_argument("--no_eval", action="store_true")
        p.add_argument("--eval_eigen_to_benchmark", action="store_true")
        p.add_argument("--eval_out_dir", type=str)
        p.add_argument("--post_process", action="store_true")
        p.add_argument("--gt_depth", action="store_true")
        # NEW: attack hyper-parameters (defaults = the values hard-coded at MD2/trainer.py:199-223)
        p.add_argument("--atk_steps", type=int, default=10)
        p.add_argument("--atk_eps", type=float, default=0.1)
        p.add_argument("--atk_alpha", type=float, default=0.02)
        p.add_argument("--atk_batch_size", type=int, default=12)
        p.add_argument("--atk_adam_lr", type=float, default=0.5)
        p.add_argument("--atk_mask_wt", type=float, default=0.06)
        p.add_argument("--atk_l0_thresh", type=float, default=0.1)
        # NEW: variant / data / distribution
        p.add_argument("--loss_variant", type=str, default="md2", choices=["md2", "dh"],
                       help="md2 = MD2/trainer.py:647-660; dh = DepthHints normalisation, DH/trainer.py:700-708")
        p.add_argument("--synthetic_len", type=int, default=64, help="items per epoch of --dataset synthetic")
        p.add_argument("--seed", type=int, default=1234)
        p.add_argument("--split_dir", type=str, default=os.path.join(file_dir, "splits"),
                       help="--dataset kitti: the folder holding <split>/train_files.txt and val_files.txt and <eval_split>/"
                            "test_files.txt -- Monodepth2's lists, which the user brings (none ships with this repository)")
        p.add_argument("--scene_root", type=str,
                       help="--dataset kitti with --adv_train: the attack's scenes (dataLoader.py:107-209), a folder with "
                            "vehicle_detection/training.txt and training/image_2/*.png of at least 375 x 1242")
        p.add_argument("--kitti_preprocess", type=str, default="reference", choices=["reference", "fast"],
                       help="--dataset kitti: reference = the loader's PIL chain on the device, bit for bit (K31: LANCZOS levels "
                            "from 8-bit levels, the 8-bit round trip of the pasted frames); fast = the synthetic set's path fed "
                            "from files (bilinear resize inside the paste, box-mean levels): NOT the reference's pixels")
        p.add_argument("--kitti_jitter", type=str, default="float", choices=["float", "pil"],
                       help="--dataset kitti with --contrastive_learning: float = ColorJitter by tensor operations on the float "
                            "level 0 (NOT the reference's pixels); pil = torchvision 0.8.2's ColorJitter on the 8-bit level 0, "
                            "Pillow's bytes, in two launches (K33); needs --kitti_preprocess reference")
        p.add_argument("--eval_gt_path", type=str,
                       help="evaluate_depth: the ground truth, an .npz with the object array ``data`` of 2-D maps (the reference "
                            "reads splits/<eval_split>/gt_depths.npz); default with --dataset synthetic: made-up LiDAR-like maps")
        p.add_argument("--eval_frames_path", type=str,
                       help="evaluate_depth: the test frames, an .npy [N, 3, 320, 1024] in [0, 1] (stands in for KITTIRAWDataset)")
        p.add_argument("--sync_attack", action="store_true",
                       help="strict reference order: wait for the gradient all-reduce + Adam before the next attack")
        p.add_argument("--shared_patch", action="store_true",
                       help="data-parallel runs: ONE patch for the whole job, as the reference's single process has (MD2/"
                            "trainer.py:300-307) -- the --atk_batch_size attack scenes are sharded over the ranks and the patch "
                            "gradient is summed over them before every sign step (SURVEY.md section 8e).  Default: every rank "
                            "attacks its own --atk_batch_size scenes and keeps its own patch (no attack-time communication)")
        p.add_argument("--materialize_warps", action="store_true",
                       help="generate_images_pred also writes depth/sample/color tensors (the fused loss never reads them)")
        p.add_argument("--use_depth_hints", action="store_true",
                       help="DepthHints (DH/options.py:99-101): depth-hint reprojection candidate + proxy supervision; needs "
                            "--loss_variant dh.  The synthetic dataset makes up hints (smooth depth with holes); --dataset kitti "
                            "reads them from --depth_hint_path (made by precompute_depth_hints.py)")
        p.add_argument("--depth_hint_path", type=str, default=None,
                       help="DepthHints (DH/options.py:102-106): the tree of precomputed hints, "
                            "<path>/<sequence>/image_0{2,3}/<frame:010d>.npy; default <data_path>/depth_hints")
        p.add_argument("--reference_stale_patch", action="store_true",
                       help="paste the adversarial patch as of the epoch start, as the reference's forked DataLoader workers "
                            "do (SURVEY.md section 3.1); default: the freshly attacked patch (its num_workers=0 behaviour)")
        p.add_argument("--no_flip_sides", action="store_true",
                       help="synthetic data: always camera side 'l' and no horizontal flips")
        p.add_argument("--pose_net", action="store_true",
                       help="build the pose networks (MD2/trainer.py:97-121) and serve the monocular frame ids of --frame_ids "
                            "(the default 0 -1 1): --pose_model_type separate_resnet / shared, --pose_model_input pairs / all; "
                            "the pose head is one HIP launch (K29).  Without it the trainer refuses monocular frame ids")
        p.add_argument("--depth_net", type=str, default="resnet", choices=["resnet", "manydepth"],
                       help="the depth network: Monodepth2's / DepthHints' ResNet U-Net (resnet), or ManyDepth's cost-volume encoder "
                            "as the reference hardens it (manydepth2/trainer.py): the degenerate single-frame call, disparities / "
                            "8.6437, built by import_depth_model(..., 'manydepth', matching=True) from --load_weights_folder (random "
                            "initialisation without one); reduce_conv runs as one HIP node (K36).  Refuses --contrastive_learning, "
                            "--pose_model_type shared, --graph_attack and --num_layers other than 18")
        p.add_argument("--max_steps", type=int, default=0, help="stop after this many iterations (0 = full epochs)")
        p.add_argument("--graph_attack", action="store_true",
                       help="L_inf attack: one set of window sizes for all steps, step 1 captured in a HIP graph and replayed "
                            "for steps 2 .. n-1 (torchattacks/attacks/phy_obj_atk.py, use_graph): takes the step's ~130 launches "
                            "off the host; for ranks whose GPU share is small (strong scaling).  L_0 attack: the same for the "
                            "fused iteration (implies --atk_fused_l0)")
        p.add_argument("--atk_fused_l0", action="store_true",
                       help="L_0 attack: the update of an iteration (mask-weight selection, both backward routes, Adam, next "
                            "compose + L0 count) as ONE launch that reads its decisions from device memory "
                            "(torchattacks/attacks/phy_obj_atk_l0.py, fused); with --graph_attack also replayed from a HIP graph")
        p.add_argument("--step_log", type=str, default="",
                       help="JSONL step log written by rank 0 (SURVEY.md section 5): one line per iteration with the loss, "
                            "images/s and the GPU time of each phase (attack / forward + loss / backward / all-reduce + "
                            "Adam) from HIP events, read one iteration late so that logging never drains the queue")
        self.parser = p

    def parse(self, args=None):
        self.options = self.parser.parse_args(args)
        if self.options.depth_hint_path is None:        # DH/trainer.py: the hints live beside the data unless told otherwise
            self.options.depth_hint_path = os.path.join(self.options.data_path, "depth_hints")
        return self.options
