"""cut_model (contrastive unpaired translation) training step on MI355X: mirror of /root/reference/models/cut_model.py
(`__init__` :216-503, `data_dependent_initialize` :505-548, `forward_cut` :611-688, `compute_G_loss_cut` :708-837,
`calculate_feats` :848-887, `calculate_NCE_loss` :889-909) and models/base_gan_model.py (`compute_D_loss(_generic)`
:341-419, `compute_G_loss_GAN(_generic)` :421-503) for the default configuration: G_netG='resnet', D_netDs=['basic'],
alg_cut_netF='mlp_sample', alg_cut_nce_loss in {'monce', 'patchnce', 'SRC_hDCE'}, nce_idt, lsgan, optionally the paired pixel loss
(alg_cut_supervised_loss 'L1' / 'MSE') and the identity pixel loss (alg_cut_MSE_idt), no semantic-mask / multimodal / temporal /
augmentation branches; data_online_context_pixels (the discriminators judge the translated crop inside its real surroundings: ops.context_split /
ops.context_frame); the semantic-consistency class branch train_semantic_cls (a classifier as third network group, ops.cls_loss); the discriminator regularisers dataaug_D_noise (Gaussian noise on both discriminator inputs) and dataaug_APA
(adaptive pseudo augmentation) run through ops.d_aug / ops.apa_update, dataaug_D_diffusion (Diffusion-GAN noise on the projected
discriminator's backbone features) inside that discriminator through ops.d_diffusion / ops.d_diffusion_update.

Per iteration (reference order): group G = {G_A, F}: fake = G(cat(real_A, real_B)); loss_G_tot = lambda_GAN * lsgan(D(fake_B), 1)
+ (NCE(real_A, fake_B) + NCE(real_B, idt_B)) / 2; backward; Adam step on G and on F (two fused launches).  Group D: fake from the
image pool, loss_D_tot = (lsgan(D(real_B), 1) + lsgan(D(fake), 0)) / 2; backward; Adam step on D.
Images are converted ONCE to NHWC 16-bit (3 -> 8 channels); every conv / norm / loss runs on the HIP kernels."""
from __future__ import annotations

import warnings

import torch

from .. import ops
from ..modules.NCE.hdce import PatchHDCELoss
from ..modules.NCE.patchnce import MoNCELoss, PatchNCELoss
from ..modules.cut_networks import PatchSampleF
from ..modules.dropout import DropoutState, FusedDropout, bind_dropout
from ..modules.resnet_generator import ResnetGenerator
from ..options import D_AUG_DEFAULTS, SEM_CLS_DEFAULTS
from ..util.image_pool import ImagePool
from .base_model import BaseModel, NetworkGroup
from .cut_step import CUTStepDriver, gate
from .gan_common import _ScaleGradFn, check_d_diffusion_options, check_discriminator_options, define_D_optimizers, define_discriminators

CUT_DEFAULTS = dict(
    alg_cut_lambda_NCE=1.0, alg_cut_lambda_SRC=0.0, alg_cut_nce_idt=True, alg_cut_nce_layers="0,4,8,12,16",
    alg_cut_nce_includes_all_negatives_from_minibatch=False, alg_cut_nce_loss="monce", alg_cut_netF="mlp_sample",
    alg_cut_netF_nc=256, alg_cut_nce_T=0.07, alg_cut_HDCE_gamma=1.0, alg_cut_HDCE_gamma_min=1.0, alg_cut_num_patches=256, alg_cut_flip_equivariance=False, alg_cut_MSE_idt=False,
    alg_cut_supervised_loss=[""], alg_cut_lambda_supervised=1.0, alg_cut_lambda_MSE_idt=1.0, alg_gan_lambda=1.0, train_gan_mode="lsgan", D_netDs=["basic"], D_ndf=64, D_n_layers=3,
    D_dropout=False, D_spectral=False, dataaug_D_label_smooth=False, dataaug_D_noise=0.0, dataaug_APA=False,
    dataaug_D_diffusion=False, dataaug_D_diffusion_every=4, train_semantic_mask=False, train_semantic_cls=False, train_mask_out_mask=False,
    **D_AUG_DEFAULTS,
)


FORK_GAN_DEFAULT = True


def check_nce_options(opt):
    """the contrastive-loss options of cut_model.py:39-137 that this build accepts; returns True for SRC_hDCE.  Host-only (no device)."""
    for k in ("alg_cut_nce_loss", "alg_cut_lambda_SRC", "alg_cut_HDCE_gamma"):
        if not hasattr(opt, k):
            setattr(opt, k, CUT_DEFAULTS[k])
    if opt.alg_cut_nce_loss not in ("monce", "patchnce", "SRC_hDCE"):
        raise NotImplementedError(f"alg_cut_nce_loss={opt.alg_cut_nce_loss!r}")
    hdce = opt.alg_cut_nce_loss == "SRC_hDCE"
    if hdce and not float(opt.alg_cut_HDCE_gamma) > 0.0:
        raise ValueError(f"alg_cut_HDCE_gamma={opt.alg_cut_HDCE_gamma!r}: the hDCE weights are exp(similarity / gamma), gamma must be > 0")
    if opt.alg_cut_lambda_SRC > 0:
        if not hdce:      # the reference builds its SRC criterion only with SRC_hDCE and fails on the missing attribute otherwise
            raise NotImplementedError("alg_cut_lambda_SRC > 0 needs alg_cut_nce_loss='SRC_hDCE'")
        # cut_model.py:734-761: loss_G_SRC is computed, reset to 0.0 (alg_cut_MSE_idt off) and never added to loss_G_tot
        warnings.warn("alg_cut_lambda_SRC > 0: as in the reference, the SRC (JSD) term does not enter the update; only the hDCE weights do")
    return hdce


def check_pixel_loss_options(opt):
    """the pixel-loss options of cut_model.py:309-319 that this build accepts; returns the ops.pixel_loss modes (supervised term, identity
    term).  "MSE" wins over "L1" when both are listed (the reference's if / elif); alg_cut_MSE_idt is an L1 loss despite its name (:309-310)
    and is off at lambda_MSE_idt <= 0 (:771).  Host-only (no device)."""
    for k in ("alg_cut_supervised_loss", "alg_cut_lambda_supervised", "alg_cut_MSE_idt", "alg_cut_lambda_MSE_idt", "alg_cut_nce_idt"):
        if not hasattr(opt, k):
            setattr(opt, k, CUT_DEFAULTS[k])
    sup = [s for s in opt.alg_cut_supervised_loss if s]
    bad = [s for s in sup if s not in ("L1", "MSE")]
    if bad:
        raise NotImplementedError(f"alg_cut_supervised_loss={bad!r}: 'L1' and 'MSE' are built ('LPIPS' / 'DISTS' need pretrained networks)")
    if opt.alg_cut_MSE_idt and not opt.alg_cut_nce_idt:      # the reference reads an idt_B that forward_cut never made
        raise ValueError("alg_cut_MSE_idt needs alg_cut_nce_idt: the identity image G(real_B) exists only with it")
    mode_sup = ops.PIXEL_MSE if "MSE" in sup else ops.PIXEL_L1 if "L1" in sup else ops.PIXEL_OFF
    mode_idt = ops.PIXEL_L1 if opt.alg_cut_MSE_idt and float(opt.alg_cut_lambda_MSE_idt) > 0.0 else ops.PIXEL_OFF
    return mode_sup, mode_idt


def check_d_aug_options(opt):
    """dataaug_D_noise (cut_model.py:668-682) and dataaug_APA (base_gan_model.py:359-365, loss.py:199-246) as this build accepts them; returns
    (sigma, apa).  Host-only (no device)."""
    for k in ("dataaug_D_noise", "dataaug_APA", *D_AUG_DEFAULTS):
        if not hasattr(opt, k):
            setattr(opt, k, CUT_DEFAULTS[k])
    sigma, apa = float(opt.dataaug_D_noise), bool(opt.dataaug_APA)
    if sigma != sigma or sigma < 0.0:
        raise ValueError(f"dataaug_D_noise={opt.dataaug_D_noise!r}: a standard deviation, >= 0")
    if apa:
        if getattr(opt, "isTrain", True) and int(getattr(opt, "train_pool_size", 50)) <= 0:      # the reference fails in ImagePool.get_random
            raise ValueError("dataaug_APA draws its substitutes from the history pool: train_pool_size must be > 0")
        if not 0.0 <= float(opt.dataaug_APA_p) <= 1.0 or int(opt.dataaug_APA_every) < 1 or not float(opt.dataaug_APA_nimg) > 0:
            raise ValueError(f"dataaug_APA_p={opt.dataaug_APA_p!r} in [0, 1], dataaug_APA_every={opt.dataaug_APA_every!r} >= 1 and "
                             f"dataaug_APA_nimg={opt.dataaug_APA_nimg!r} > 0 are required")
        if len(opt.D_netDs) > ops.D_AUG_MAX:
            raise NotImplementedError(f"dataaug_APA with more than {ops.D_AUG_MAX} discriminators")
    return sigma, apa


CONTEXT_VISUAL_NAMES = ["real_A_with_context_vis", "real_B_with_context_vis", "fake_B_with_context_vis", "mask_context_vis"]      # cut_model.py:485-490


def check_context_options(opt):
    """data_online_context_pixels (base_model.py:134 `margin`, :389-431 set_input, :609-636 compute_fake_with_context; base_gan_model.py:186-215
    mask_context) as this build accepts it; returns c, the width of the frame the discriminators see around the crop (0: off).  The reference
    multiplies a mask of model_input_nc channels into an image of model_output_nc channels: the two must agree.  Host-only (no device)."""
    import numbers

    if not hasattr(opt, "data_online_context_pixels"):
        opt.data_online_context_pixels = 0
    c = opt.data_online_context_pixels
    if isinstance(c, bool) or not isinstance(c, numbers.Integral) or c < 0:
        raise ValueError(f"data_online_context_pixels={c!r}: an integer >= 0 is required")
    c = int(c)
    if c > 0 and getattr(opt, "model_input_nc", 3) != getattr(opt, "model_output_nc", 3):
        raise ValueError(f"data_online_context_pixels={c}: the frame of real_A surrounds fake_B: model_input_nc={opt.model_input_nc!r} must equal "
                         f"model_output_nc={opt.model_output_nc!r}")
    return c


def check_context_discriminators(opt, c):
    """the discriminators run on (data_crop_size + 2 c)^2 images (gan_networks.py:349-415).  The PatchGAN takes any size; the projected
    discriminators resize to D_proj_interp first, and without it their feature network is built for the framed size, which its four strides
    must divide.  Host-only (no device)."""
    size = int(opt.data_crop_size) + 2 * c
    if c > 0 and "projected_d" in opt.D_netDs and int(getattr(opt, "D_proj_interp", -1)) <= 0 and size % 32:
        raise NotImplementedError(f"data_online_context_pixels={c} with projected_d and no D_proj_interp: the framed size {size} is not a multiple "
                                  "of 32 (the feature network's deepest stride); set D_proj_interp or choose c so that it is")


DROPOUT_GENERATORS = ("resnet", "resnet_9blocks", "resnet_6blocks")      # gan_networks.py:112-122: the only G_netG that receive G_dropout


def check_dropout_options(opt):
    """G_dropout / D_dropout (nn.Dropout(0.5) in every ResnetBlock: resnet_generator.py:62-88; behind every LeakyReLU of the PatchGAN:
    discriminators.py:51-108) as this build accepts them; returns (generator dropout, PatchGAN dropout).  The reference hands G_dropout to the
    plain ResNet generator only: for every other G_netG it is ignored there and, with a warning, here.  projected_d has no dropout in the
    reference: D_dropout reaches the 'basic' discriminator only.  The value of G_dropout is not a rate: the networks use 0.5.  Host-only
    (no device)."""
    for k in ("G_dropout", "D_dropout", "D_netDs"):
        if not hasattr(opt, k):
            setattr(opt, k, CUT_DEFAULTS.get(k, False))
    g, d = bool(opt.G_dropout), bool(opt.D_dropout)
    if g and getattr(opt, "G_netG", "resnet") not in DROPOUT_GENERATORS:
        warnings.warn(f"G_dropout has no effect: G_netG={opt.G_netG!r} is not handed it (only {DROPOUT_GENERATORS} are, as in the reference)")
        g = False
    if d and "basic" not in opt.D_netDs:
        warnings.warn(f"D_dropout has no effect: D_netDs={opt.D_netDs!r} holds no 'basic' discriminator")
        d = False
    return g, d


SEM_CLS_MODES = {"CE": ops.CLS_CE, "MSE": ops.CLS_MSE, "L1": ops.CLS_L1}      # check_sem_cls_options -> mode of ops.cls_loss


def check_sem_cls_options(opt):
    """train_semantic_cls (base_model.py:208-265 init_semantic_cls, semantic_networks.py:19-42 define_C) as this build accepts it: fills the
    defaults and returns "off", or the criterion "CE" (CrossEntropyLoss), "MSE" / "L1" (train_cls_regression [+ train_cls_l1_regression]).
    Host-only (no device).  train_sem_use_label_B, cls_class_weights, cls_all_classes_as_one and cls_dropout never reach the training step of
    the reference (the data loader and the torchvision templates read them): accepted and ignored."""
    for k, v in SEM_CLS_DEFAULTS.items():
        if not hasattr(opt, k):
            setattr(opt, k, v)
    if not getattr(opt, "train_semantic_cls", False):
        return "off"
    if opt.train_sem_cls_template != "basic":
        raise NotImplementedError(f"train_sem_cls_template={opt.train_sem_cls_template!r}: 'basic' is built (the others are torchvision models)")
    if opt.train_sem_idt:      # base_gan_model.py:715-717 reads self.criterioncls and pred_cls_idt_B, which nothing creates
        raise NotImplementedError("train_sem_idt with train_semantic_cls: the reference cannot run it either (its identity class term reads "
                                  "attributes that are never set)")
    size = int(opt.data_crop_size)
    if size < 8 or size & (size - 1):      # classifiers.py:24-47: only a power of two reaches the 1x1 map its first Linear expects
        raise ValueError(f"train_semantic_cls: data_crop_size={opt.data_crop_size!r} must be a power of two >= 8")
    if opt.model_input_nc != opt.model_output_nc:
        raise ValueError(f"train_semantic_cls: one classifier sees real_A and fake_B: model_input_nc={opt.model_input_nc!r} must equal "
                         f"model_output_nc={opt.model_output_nc!r}")
    n = int(getattr(opt, "cls_semantic_nclasses", 2))
    if n < 1:
        raise ValueError(f"cls_semantic_nclasses={n!r}: >= 1 is required")
    if opt.train_cls_regression and n != 1:
        raise ValueError(f"train_cls_regression predicts one value per image: cls_semantic_nclasses={n!r} must be 1")
    if not opt.train_cls_regression:
        return "CE"
    return "L1" if opt.train_cls_l1_regression else "MSE"


def cut_loss_names(opt, discriminators_names):
    """loss_names of the generator group in the reference's order (cut_model.py:444-455): G_tot, G_NCE, [G_supervised], [G_NCE_Y], [G_MSE_idt],
    G_GAN_*, [G_sem_cls_AB] (base_model.py:212-224, appended last).  Host-only (no device)."""
    names = ["G_tot", "G_NCE"]
    if [s for s in getattr(opt, "alg_cut_supervised_loss", [""]) if s]:
        names.append("G_supervised")
    if getattr(opt, "alg_cut_nce_idt", True):
        names.append("G_NCE_Y")
    if getattr(opt, "alg_cut_MSE_idt", False):
        names.append("G_MSE_idt")
    names += ["G_GAN_" + dn for dn in discriminators_names]
    if getattr(opt, "train_semantic_cls", False):
        names.append("G_sem_cls_AB")
    return names


def cut_all_loss_names(opt, discriminators_names):
    """loss_names of the model in the reference's order: the generator's, the discriminators', then with train_semantic_cls G_sem_cls_AB and
    CLS (cut_model.py:479 joins G and D before base_model.py:224-226 appends the class names to loss_names_G and to loss_names: the two come
    AFTER the discriminators' names here, G_sem_cls_AB last in loss_names_G).  Host-only (no device)."""
    names = [n for n in cut_loss_names(opt, discriminators_names) if n != "G_sem_cls_AB"] + ["D_tot"] + ["D_GAN_" + dn for dn in discriminators_names]
    if getattr(opt, "train_semantic_cls", False):
        names += ["G_sem_cls_AB", "CLS"]
    return names


class CUTModel(BaseModel):
    def __init__(self, opt, rank):
        for k, v in CUT_DEFAULTS.items():
            if not hasattr(opt, k):
                setattr(opt, k, v)
        super().__init__(opt, rank)
        self.driver = CUTStepDriver(self)      # streams, captured graphs and the early-D order of optimize_parameters (cut_step.py)
        if self.act_dtype == torch.float16 and not float(getattr(opt, "jg_loss_scale", 0.0) or 0.0):
            # the 1/T = 14x of the contrastive logits makes these gradients ~2 orders larger than the diffusion path's:
            # 65536 overflows fp16 activation gradients, 1024 keeps both ends of the range
            self.loss_scale = 1024.0
        if opt.G_netG not in ("resnet", "resnet_9blocks", "resnet_6blocks", "segformer_attn_conv", "resnet_attn", "mobile_resnet_attn"):
            raise NotImplementedError(f"G_netG={opt.G_netG!r}: the CUT path is built for the resnet, resnet_attn, mobile_resnet_attn and "
                                      "segformer_attn_conv generators")
        if "segformer" in opt.G_netG:           # cut_model.py:205-210: enforced by the reference
            opt.alg_cut_nce_layers, opt.alg_cut_nce_T = "0,1,2,3", 0.2
        check_discriminator_options(opt)
        if opt.alg_cut_netF != "mlp_sample":
            raise NotImplementedError(f"alg_cut_netF={opt.alg_cut_netF!r}")
        self.hdce = check_nce_options(opt)
        self.pixel_modes = check_pixel_loss_options(opt)      # (supervised term, identity term) of ops.pixel_loss
        for flag in ("model_multimodal", "alg_cut_flip_equivariance", "train_semantic_mask", "train_mask_out_mask"):
            if getattr(opt, flag, False):
                raise NotImplementedError(f"{flag} is outside the SURVEY.md 8 hot path")
        check_d_aug_options(opt)
        self.context = check_context_options(opt)      # c of data_online_context_pixels: 0 = off
        check_context_discriminators(opt, self.context)
        self.sem_cls = check_sem_cls_options(opt)      # "off" | "CE" | "MSE" | "L1"
        # dataaug_D_diffusion: the projected discriminator noises its own backbone features (modules/projected_d.Diffusion) and its loss
        # calculator moves the strength; nothing of it lives in this model
        self.d_diffusion = check_d_diffusion_options(opt)
        self.loss_G_SRC = 0.0      # cut_model.py:734-761: computed there, never part of loss_G_tot; not computed here
        # cut_model.py:752-766: with alg_cut_MSE_idt the identity contrastive term of SRC_hDCE runs with the hDCE weights too
        self.hdce_idt_weighted = bool(self.hdce and opt.alg_cut_MSE_idt)
        # options that select ANOTHER network than the one built here must not be dropped silently: the generator /
        # PatchGAN below are the InstanceNorm, no-spectral-norm variants of gan_networks.define_G / define_D
        self.g_dropout, self.d_dropout = check_dropout_options(opt)
        for name, built in (("D_spectral", False), ("G_spectral", False), ("G_norm", "instance"), ("D_norm", "instance")):
            val = getattr(opt, name, built)
            if val != built and not (name.endswith("_norm") and "segformer" in opt.G_netG and name == "G_norm"):
                raise NotImplementedError(f"{name}={val!r}: only {built!r} is built for the CUT networks")
        self.nce_layers = [int(i) for i in str(opt.alg_cut_nce_layers).split(",")]
        if "segformer" in opt.G_netG:            # gan_networks.py:177-187
            from ..modules.segformer import SegformerGenerator_attn

            self.netG_A = SegformerGenerator_attn(getattr(opt, "jg_dir", ""), getattr(opt, "G_config_segformer", ""), opt.model_input_nc,
                                                  img_size=opt.data_crop_size, nb_mask_attn=getattr(opt, "G_attn_nb_mask_attn", 10),
                                                  nb_mask_input=getattr(opt, "G_attn_nb_mask_input", 1), final_conv=True,
                                                  padding_type=opt.G_padding_type)
        elif "resnet_attn" in opt.G_netG:        # gan_networks.py:150-176
            from ..modules.resnet_attn_generator import ResnetGenerator_attn

            if getattr(opt, "train_feat_wavelet", False):
                raise NotImplementedError("train_feat_wavelet (wavelet feature space) is outside the built path")
            self.netG_A = ResnetGenerator_attn(opt.model_input_nc, opt.model_output_nc, getattr(opt, "G_attn_nb_mask_attn", 10),
                                               getattr(opt, "G_attn_nb_mask_input", 1), opt.G_ngf, n_blocks=opt.G_nblocks,
                                               padding_type=opt.G_padding_type, mobile=opt.G_netG.startswith("mobile"),
                                               twice_resnet_blocks=getattr(opt, "G_backward_compatibility_twice_resnet_blocks", False))
        else:
            self.netG_A = ResnetGenerator(opt.model_input_nc, opt.model_output_nc, opt.G_ngf, n_blocks=opt.G_nblocks,
                                          padding_type=opt.G_padding_type, use_dropout=self.g_dropout)
        self.model_names = ["G_A"]
        if opt.isTrain:
            self.netF = PatchSampleF(use_mlp=True, init_type=opt.model_init_type, init_gain=opt.model_init_gain, nc=opt.alg_cut_netF_nc)
            self.netF.set_device(self.device)
            self.discriminators_names = define_discriminators(self, opt)
            self.model_names += ["F"] + self.discriminators_names
            # base_model.py:115-118; forward_GAN (base_gan_model.py:170-173) also pushes the real images through pools on every
            # iteration: they feed only the metrics, but they consume host random draws BEFORE the fake pool does
            self.real_A_pool, self.real_B_pool = ImagePool(opt.train_pool_size), ImagePool(opt.train_pool_size)
            self.fake_B_pool = ImagePool(opt.train_pool_size)
            crit = PatchHDCELoss if self.hdce else MoNCELoss if opt.alg_cut_nce_loss == "monce" else PatchNCELoss
            self.criterionNCE = [crit(opt) for _ in self.nce_layers]
            kw = dict(lr=opt.train_G_lr, betas=(opt.train_beta1, opt.train_beta2), weight_decay=opt.train_optim_weight_decay,
                      eps=opt.train_optim_eps)
            self.optimizer_G = self.make_optimizer(self.netG_A, **kw)
            kw["lr"] = opt.train_D_lr
            optD = define_D_optimizers(self, opt, kw)
            self.optimizers.append(self.optimizer_G)
            self.group_G = NetworkGroup(networks_to_optimize=["G_A", "F"], forward_functions=["forward"],
                                        backward_functions=["compute_G_loss"], loss_names_list=["loss_names_G"],
                                        optimizer=["optimizer_G", "optimizer_F"], loss_backward=["loss_G_tot"], networks_to_ema=["G_A"])
            self.group_D = NetworkGroup(networks_to_optimize=list(self.discriminators_names), forward_functions=None,
                                        backward_functions=["compute_D_loss"], loss_names_list=["loss_names_D"], optimizer=optD,
                                        loss_backward=["loss_D_tot"])
            self.networks_groups = [self.group_G, self.group_D]
            self.loss_names_G = cut_loss_names(opt, self.discriminators_names)
            self.loss_names_D = ["D_tot"] + ["D_GAN_" + dn for dn in self.discriminators_names]
            self.loss_names = cut_all_loss_names(opt, self.discriminators_names)
            self.loss_functions_G = ["compute_G_loss_GAN", "compute_G_loss_cut"]
            if self.sem_cls != "off":
                self.init_semantic_cls(opt, kw)
            self.iter_calculator_init()
        else:
            self.netG_A.jg_finalize(self.device, self.act_dtype)
        self.patch_ids_injection = None   # parity runs: callable(call_index, feat_shapes) -> list of id tensors
        # parity runs: callable(kind, index) -> the draws of dataaug_D_noise / dataaug_APA as the reference makes them, or None (drawn in the
        # kernel): ("z_fake", 0) / ("z_real", 0): fp32 [B, C, H, W] of torch.normal(0, 1);  ("u", d): fp32 [B] of discriminator d's torch.rand
        self.d_aug_injection = None
        self.d_noise, self.d_apa = check_d_aug_options(opt)
        if self.d_apa and opt.isTrain:
            self.visual_names.append(["APA_img"])
        if self.context:
            # cut_model.py:483-492: the framed images resized to the crop; made on demand (compute_visuals), not per step
            self.context_visual_names = list(CONTEXT_VISUAL_NAMES)
            self.visual_names.append(self.context_visual_names)
            # the Philox key of the step's dataaug_D_noise: the frame launch of the forward draws the fake batch's noise with it (inside the
            # captured generator graph), the discriminator half the real batch's -- one buffer, refilled in place, as the dropout key is
            self._ctx_key = torch.zeros(2, device=self.device, dtype=torch.int32) if self.d_noise > 0.0 and opt.isTrain else None
        self._bind_dropout()

    # ---- G_dropout / D_dropout ------------------------------------------------------------------------------------------------------------
    def _bind_dropout(self):
        """One DropoutState for the generator and every discriminator: unique Philox streams across them, module paths `netG_A.encoder...` /
        `netD_B_basic.model...`, ONE key per step.  The key lives in a buffer of the model's own that the step refills in place
        (`_forward_core`, inside the captured region), so that the generator graphs and the discriminator graph read the same address."""
        self.dropout_state = DropoutState()
        nets = [("netG_A", self.netG_A)] + [("net" + dn, getattr(self, "net" + dn)) for dn in getattr(self, "discriminators_names", [])]
        n = 0
        for name, net in nets:
            if hasattr(net, "dropout_state"):
                n = bind_dropout(net, self.dropout_state, name + ".", n)
        self._dropout_on = n > 0
        self._drop_key = torch.zeros(2, device=self.device, dtype=torch.int32) if self._dropout_on else None

    @property
    def dropout_rand(self):
        """parity runs: callable(module_path, call, shape_BCHW, device) -> the fp32 uniforms of that invocation of that Dropout module"""
        return self.dropout_state.rand

    @dropout_rand.setter
    def dropout_rand(self, fn):
        self.dropout_state.rand = fn

    def _dropout_seek(self, names, call):
        """the next invocation of every Dropout module of the networks `names` is `call`: the discriminators run once in the generator's loss
        (call 0) and then in their own half (from call 1), whichever driver enqueues the halves and whether or not a half is replayed"""
        if self._dropout_on:
            for nm in names:
                for m in self._net(nm).modules():
                    if isinstance(m, FusedDropout):
                        self.dropout_state.calls[m.stream] = call

    # ---- semantic-consistency class branch (train_semantic_cls) -------------------------------------------------------------------------
    def init_semantic_cls(self, opt, kw):
        """base_model.py:208-265: netCLS, its criterion and optimizer, and the third network group [G, D, CLS]."""
        from ..modules.classifier import Classifier

        self.netCLS = Classifier(opt.model_output_nc, opt.cls_nf, opt.cls_semantic_nclasses, opt.data_crop_size, init_type=opt.model_init_type,
                                 init_gain=opt.model_init_gain)
        self.model_names += ["CLS"]
        self.loss_names_CLS = ["CLS"]
        # base_model.py:237-244: the reference builds this optimizer with train_sem_lr_f_s -- train_sem_lr_cls is never read.  Its slip, mirrored.
        self.optimizer_CLS = self.make_optimizer(self.netCLS, **{**kw, "lr": opt.train_sem_lr_f_s})
        self.optimizers.append(self.optimizer_CLS)
        self.group_CLS = NetworkGroup(networks_to_optimize=["CLS"], forward_functions=None, backward_functions=["compute_CLS_loss"],
                                      loss_names_list=["loss_names_CLS"], optimizer=["optimizer_CLS"], loss_backward=["loss_CLS"])
        self.networks_groups.append(self.group_CLS)
        self.loss_functions_G.insert(1, "compute_G_loss_semantic_cls")      # base_gan_model.py:151-153, cut_model.py:499: GAN, class, CUT
        # the gate of the generator's class term (base_gan_model.py:719-724) reads LAST iteration's loss_CLS: kept as a device scalar that the
        # classifier step's loss launch writes and the generator's launch reads -- no host synchronisation.  +inf = "no loss_CLS yet": closed.
        self.loss_CLS_prev = torch.full((), float("inf"), device=self.device, dtype=torch.float32)

    def sem_cls_gate_open(self):
        """whether the NEXT generator step's class term is let through (a host read of the device scalar: logging and tests only)"""
        return not float(self.loss_CLS_prev) > float(self.opt.f_s_semantic_threshold)

    def _set_input_semantic_cls(self, data):
        """base_model.py:476-494: A_label_cls (long; float in regression mode) and, if present, B_label_cls.  The range check runs here, where
        the labels are still on the host: the kernel turns a bad label into a NaN loss, this turns it into an error."""
        regression = self.sem_cls != "CE"
        n = int(self.opt.cls_semantic_nclasses)
        for dom in ("A", "B"):
            key = dom + "_label_cls"
            if key not in data:
                if dom == "A" or self.opt.train_sem_cls_B:
                    raise KeyError(f"train_semantic_cls{' with train_sem_cls_B' if dom == 'B' else ''} needs data[{key!r}]")
                continue
            lab = torch.as_tensor(data[key]).reshape(-1)
            if not regression and not lab.is_cuda and lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= n):
                raise ValueError(f"{key} holds a class outside [0, {n}): {lab.tolist()}")
            lab = lab.to(torch.float32 if regression else torch.int64)
            setattr(self, f"input_{dom}_label_cls", lab.to(self.device, non_blocking=True).contiguous())

    def forward_semantic_cls(self):
        """base_model.py:1618-1635: netCLS(real_A) then netCLS(fake_B), both in train mode: each pass normalises with its batch statistics and
        updates the running ones (the third pass of the iteration is compute_CLS_loss).  The argmaxes of the reference (gt_pred_cls_A / pfB)
        come out of the loss launches on the same logits: pfB from the generator's term, gt_pred_cls_A from the classifier's (its pass on
        real_A sees the same weights and batch statistics as this one)."""
        net = self._net("CLS")
        self.pred_cls_real_A = net(self.real_A)
        self.pred_cls_fake_B = net(self.fake_B)

    def compute_G_loss_semantic_cls(self):
        """base_gan_model.py:686-737: lambda * gate * criterion(netCLS(fake_B), label_A); the gate reads f_s_semantic_threshold (the reference's
        slip: cls_semantic_threshold is never read; mirrored) against last iteration's loss_CLS on the device."""
        o = self.opt
        self.loss_G_sem_cls_AB, self.pfB = ops.cls_loss(self.pred_cls_fake_B, self.input_A_label_cls, SEM_CLS_MODES[self.sem_cls], o.train_sem_cls_lambda,
                                                        prev=self.loss_CLS_prev, threshold=o.f_s_semantic_threshold)
        self.loss_G_tot = self.loss_G_tot + self.loss_G_sem_cls_AB

    def compute_CLS_loss(self):
        """base_model.py:1497-1520: lambda * criterion(netCLS(real_A), label_A) [+ the same on real_B with train_sem_cls_B], ungated; the
        launch(es) leave the value in loss_CLS_prev for the next iteration's gate."""
        o = self.opt
        net, mode = self._net("CLS"), SEM_CLS_MODES[self.sem_cls]
        loss, self.gt_pred_cls_A = ops.cls_loss(net(self.real_A), self.input_A_label_cls, mode, o.train_sem_cls_lambda, state=self.loss_CLS_prev)
        if o.train_sem_cls_B:
            loss_B, self.gt_pred_cls_B = ops.cls_loss(net(self.real_B), self.input_B_label_cls, mode, o.train_sem_cls_lambda, state=self.loss_CLS_prev,
                                                      state_acc=True)
            loss = loss + loss_B
        self.loss_CLS = _ScaleGradFn.apply(loss, self.loss_scale)

    def parallelize(self, rank):
        if self.sem_cls != "off" and len(self.opt.gpu_ids) > 1:
            raise NotImplementedError("train_semantic_cls on more than one GPU: the classifier's synchronised BatchNorm statistics over its three "
                                      "passes and a third arena in the gradient exchange are not built")
        super().parallelize(rank)

    # ---- inputs ---------------------------------------------------------------------------------------------------
    def set_input(self, data):
        c = self.context
        if c > 0:
            # base_model.py:389-431: the loader hands over images 2 c larger than the crop; the generator group reads the centre crops
            # (real_A / real_B), the discriminators the whole images (real_*_with_context).  One launch per domain writes both.
            S = int(self.opt.data_crop_size)
            for dom in ("A", "B"):
                shape = tuple(data[dom].shape)
                if len(shape) != 4 or shape[2:] != (S + 2 * c, S + 2 * c):
                    raise ValueError(f"data_online_context_pixels={c}: data[{dom!r}] must be [B, C, {S + 2 * c}, {S + 2 * c}] (data_crop_size {S} "
                                     f"+ 2 x {c} context pixels), got {shape}")
                full = data[dom].to(self.device, non_blocking=True).float()
                framed, crop = ops.context_split(full, c, self.act_dtype)
                setattr(self, f"real_{dom}_with_context_nchw", full)
                setattr(self, f"real_{dom}_nchw", full[:, :, c:-c, c:-c])      # the fp32 centre view
                setattr(self, f"real_{dom}_with_context", framed)
                setattr(self, f"real_{dom}", crop)
        else:
            self.real_A_nchw = data["A"].to(self.device, non_blocking=True)
            self.real_B_nchw = data["B"].to(self.device, non_blocking=True)
            self.real_A = ops.to_nhwc(self.real_A_nchw, self.act_dtype)
            self.real_B = ops.to_nhwc(self.real_B_nchw, self.act_dtype)
        self.batch_size = self.real_A.shape[0]
        if self.sem_cls != "off" and self.opt.isTrain:
            self._set_input_semantic_cls(data)

    def get_current_batch_size(self):
        return self.batch_size

    def data_dependent_initialize(self, data):
        """cut_model.py:505-548: the MLP widths of netF come from the tapped feature widths; optimizer_F is created here."""
        self.set_input(data)
        if self.opt.isTrain:
            self.feat_channels = self.netG_A.feat_channels(self.nce_layers)
            self.netF.data_dependent_initialize(None, self.feat_channels)
            self.optimizer_F = self.make_optimizer(self.netF, lr=self.opt.train_G_lr, betas=(self.opt.train_beta1, self.opt.train_beta2),
                                                   weight_decay=self.opt.train_optim_weight_decay, eps=self.opt.train_optim_eps)
            self.optimizers.append(self.optimizer_F)
        for o in self.optimizers:
            o.zero_grad()

    # ---- forward (cut_model.py:611-688) ---------------------------------------------------------------------------
    def set_pool_rng(self, rng):
        """parity runs: one host RNG (uniform / randint) shared by the three pools, like the reference's `random` module."""
        for p in (self.real_A_pool, self.real_B_pool, self.fake_B_pool):
            p.rng = rng

    def forward(self):
        if self.opt.isTrain:
            self.real_A_pool.store(self.real_A)
            self.real_B_pool.store(self.real_B)
        self._forward_core()
        if self.sem_cls != "off" and self.opt.isTrain:
            self.forward_semantic_cls()

    def _reuse_feats(self):
        """`jg_nce_reuse_feats` (round 6, default on): the key-side features of both contrastive terms -- `netG.get_feats` of the source image
        (NCE term) and of the target image (identity term), cut_model.py:848-887 -- are the encoder activations the generator's forward has
        just computed on cat(real_A, real_B): for an encoder that is a deterministic function of its input in training mode (the ResNet
        families: InstanceNorm, no dropout) a second pass recomputes the same values from the same weights, and its backward adds the same
        gradients to them.  The forward hands the tapped activations out (`forward_with_feats`) and the encoder pass of the loss runs over the
        2 B translated / identity images only.  NOT for the SegFormer encoder: its DropPath masks are drawn per pass in the reference."""
        net = self._net("G_A")
        return (gate(self.opt, "jg_nce_reuse_feats", "JG_NCE_REUSE_FEATS") and self.opt.isTrain and getattr(net, "deterministic_encoder", False)
                and net.training and self._batched_nce())

    def _forward_core(self):
        B = self.batch_size
        self.real = torch.cat((self.real_A, self.real_B), dim=0) if self.opt.alg_cut_nce_idt else self.real_A
        self._real_feats = None
        if self._dropout_on and self.opt.isTrain:
            # a new step for every Dropout module: invocation counts back to 0 and one fresh Philox key, drawn on the device into the model's
            # own buffer (inside the generator graph when the step is captured, as the key of dataaug_D_noise is inside its region)
            if self.dropout_state.rand is None:
                self._drop_key.copy_(ops.d_aug_key(self.device))
            self.dropout_state.begin_step(self._drop_key)
        if self._reuse_feats():
            self.fake, self._real_feats = self._net("G_A").forward_with_feats(self.real, self.nce_layers)
        else:
            self.fake = self._net("G_A")(self.real)
        self.fake_B = self.fake[:B]
        if self.context:
            self._frame_fake()
        if self.opt.alg_cut_nce_idt:
            self.idt_B = self.fake[B:]
        self._feat_calls = 0

    # ---- data_online_context_pixels ---------------------------------------------------------------------------------------------------------
    @property
    def real_B_D(self):
        """the real image as the discriminators see it"""
        return self.real_B_with_context if self.context else self.real_B

    @property
    def fake_B_D(self):
        """the translated image as the discriminators see it (with the generator's autograd history)"""
        return self.fake_B_with_context if self.context else self.fake_B

    def _frame_fake(self):
        """compute_fake_with_context (base_model.py:609-636) and, with dataaug_D_noise, the noisy copy of the framed fake (cut_model.py:668-682)
        from ONE launch: fake_B_with_context carries the generator's gradient into the GAN terms, fake_B_with_context_noisy (detached) goes to
        the history pool.  The fake batch is drawn first (call index 0), the real batch later by real_D_operands (call index 1) on the same
        key: the reference's draw order.  The key is drawn here, on the device, into the model's own buffer -- inside graph F when the step
        is captured."""
        sigma = self.d_noise if self.opt.isTrain else 0.0
        z = key = None
        if sigma > 0.0:
            z = self.frame_noise_injection(refresh=not torch.cuda.is_current_stream_capturing())
            if z is None:
                self._ctx_key.copy_(ops.d_aug_key(self.device))
                key = self._ctx_key
            self._d_key = key
        self.fake_B_with_context, noisy = ops.context_frame(self.fake_B, self.real_A_with_context, self.context, self.opt.model_output_nc, sigma,
                                                            z=z, key=key, call=0)
        if sigma > 0.0:
            self.fake_B_with_context_noisy = noisy

    def frame_noise_injection(self, refresh=True):
        """parity runs: the injected z of the framed fake batch (`d_aug_injection("z_fake")`) in a buffer of the model's own, one per shape,
        so that a captured graph F reads the same address at every replay; `refresh` copies this step's draw into it (the step driver does
        that ahead of a replay, the eager forward here).  None without an injection: the kernel draws."""
        if not (self.context and self.d_noise > 0.0 and self.opt.isTrain) or self.d_aug_injection is None:
            return None
        if not refresh:
            return self._ctx_z[self._ctx_z_shape]
        z = self._d_aug_draw("z_fake")
        if not hasattr(self, "_ctx_z"):
            self._ctx_z = {}
        self._ctx_z_shape = tuple(z.shape)
        buf = self._ctx_z.get(self._ctx_z_shape)
        if buf is None:
            buf = self._ctx_z[self._ctx_z_shape] = torch.empty(self._ctx_z_shape, device=self.device, dtype=torch.float32)
        buf.copy_(z)
        return buf

    def compute_visuals(self, nb_imgs):
        """the context visuals of the reference (cut_model.py:483-492), made when the display asks for them: the framed images and the mask
        resized to the crop by nearest F.interpolate, fp32 NCHW as the reference's are"""
        super().compute_visuals(nb_imgs)
        if not self.context or not hasattr(self, "real_A_with_context_nchw"):
            return
        import torch.nn.functional as F

        c, size = self.context, tuple(self.real_A_nchw.shape[2:])
        self.real_A_with_context_vis = F.interpolate(self.real_A_with_context_nchw, size=size)
        self.real_B_with_context_vis = F.interpolate(self.real_B_with_context_nchw, size=size)
        if hasattr(self, "fake_B_with_context"):
            self.fake_B_with_context_vis = F.interpolate(ops.to_nchw_f32(self.fake_B_with_context.detach(), self.opt.model_output_nc), size=size)
        mask = torch.ones_like(self.real_A_with_context_nchw)      # base_gan_model.py:186-215
        mask[:, :, c:-c, c:-c] = 0.0
        self.mask_context_vis = F.interpolate(mask, size=size)[:, 0]

    # ---- generator losses ---------------------------------------------------------------------------------------------
    def _fork_gan(self):
        """`JG_FORK_GAN` / option `jg_fork_gan` (round 6): the two branches of the generator loss hang off `fake_B` independently -- the GAN terms
        (every discriminator's forward on the translated image, ViT projector included) and the contrastive terms (encoder passes, PatchSampleF,
        NCE) -- and each is a string of 5 - 30 us launches that fills a fraction of the chip.  The GAN branch is enqueued on a forked stream;
        autograd runs a node's backward on the stream of its forward, so the two branches overlap in the backward as well, and both forks are
        captured into the generator graphs (a fork that joins before the capture ends is a legal capture)."""
        return (gate(self.opt, "jg_fork_gan", "JG_FORK_GAN", FORK_GAN_DEFAULT, force=True) and self.device.type == "cuda" and not ops.TORCH_OPS_BOUNDARY
                and ops.KERNEL_TIMING is None and "compute_G_loss_GAN" in self.loss_functions_G and len(self.loss_functions_G) > 1)

    def compute_G_loss(self):
        self.loss_G_tot = 0
        if self._fork_gan():
            main = torch.cuda.current_stream(self.device)
            side = self.driver.stream("gan_stream")
            side.wait_stream(main)
            for t in (self.fake_B_D, self.real_B_D):
                t.record_stream(side)
            with torch.cuda.stream(side):
                self.compute_G_loss_GAN()
                gan_tot, self.loss_G_tot = self.loss_G_tot, 0
            for f in self.loss_functions_G:
                if f != "compute_G_loss_GAN":
                    getattr(self, f)()
            main.wait_stream(side)
            gan_tot.record_stream(main)
            for dn in self.discriminators_names:
                getattr(self, "loss_G_GAN_" + dn).record_stream(main)
            self.loss_G_tot = self.loss_G_tot + gan_tot
        else:
            for f in self.loss_functions_G:
                getattr(self, f)()
        self.loss_G_tot = _ScaleGradFn.apply(self.loss_G_tot, self.loss_scale)

    def compute_G_loss_GAN(self):
        """base_gan_model.py:421-503: lambda_GAN * compute_loss_G of every discriminator on domain B."""
        self._dropout_seek(self.discriminators_names, 0)
        for dn in self.discriminators_names:
            lossf = getattr(self, dn + "_loss_calculator")
            val = self.opt.alg_gan_lambda * lossf.compute_loss_G(self._net(dn), self.real_B_D, self.fake_B_D)
            setattr(self, "loss_G_GAN_" + dn, val)
            self.loss_G_tot = self.loss_G_tot + val

    def _batched_nce(self):
        """one encoder pass / one PatchSampleF pass / one NCE launch set for BOTH contrastive terms (`jg_batched_nce`, default on): needs the
        identity term, an un-injected random source (parity runs inject per-call draws in the reference's order) and the per-image negatives"""
        o = self.opt
        net = self._net("G_A")
        if self.g_dropout:      # the reference draws a fresh mask in each of its four encoder passes: the same passes, the same (stream, call) pairs
            return False
        return (gate(o, "jg_batched_nce", "JG_BATCHED_NCE") and o.alg_cut_nce_idt and o.alg_cut_lambda_NCE > 0.0
                and self.patch_ids_injection is None and getattr(getattr(net, "rand", None), "source", None) is None
                and not o.alg_cut_nce_includes_all_negatives_from_minibatch and not ops.TORCH_OPS_BOUNDARY)

    def compute_G_loss_cut_batched(self):
        """cut_model.py:708-909 with the four encoder passes (translated / source image of the NCE term, identity / target image of the identity
        term), the four PatchSampleF passes and the 2 x L contrastive problems each run ONCE on the concatenated batch (round 5).  The reference
        calls `netG.get_feats` four times on B images and `netF` four times; the encoder is per-sample (LayerNorm / InstanceNorm, DropPath draws
        per sample) and netF's MLPs are per-row, so one pass over 4 B images computes the same features -- with a quarter of the launches, on
        problems four times the size.  Patch ids: one draw per (term, layer) in the reference's order (the source-image pass draws, the translated
        image reuses them, cut_networks.py:57-60).  The L problems of a term that share a patch count, and the two terms, are one batched
        PatchNCE / MoNCE call (images are independent problems in every kernel: the 50 Sinkhorn iterations of 2 L x B images run side by side
        instead of in 2 L launches of B)."""
        o = self.opt
        B = self.batch_size
        net, netF = self._net("G_A"), self._net("F")
        # images in the order [translated | identity | source | target] = cat(G's output, G's input): no slice of either is needed, and the
        # rows of every layer come out as [q of term 0 | q of term 1 | k of term 0 | k of term 1]
        reuse = getattr(self, "_real_feats", None)
        if reuse is not None:         # `jg_nce_reuse_feats`: the source / target features are the forward's own activations
            feats = net.get_feats(self.fake, self.nce_layers)
            feats_k, self._real_feats = reuse, None
        else:
            feats = net.get_feats(torch.cat((self.fake, self.real), dim=0), self.nce_layers)
            feats_k = None
        self._feat_calls += 2
        netF.arena.ensure_fresh()
        P = o.alg_cut_num_patches
        rows, counts = [], []
        ids_all = [[netF.draw_ids(f, P) for f in feats] for _ in range(2)]         # term 0: NCE, term 1: identity NCE (reference draw order)
        for li, f in enumerate(feats):
            C = self.feat_channels[li]
            ids = torch.stack((ids_all[0][li], ids_all[1][li]))                      # [2, P_l]: images b use set (b // B) % 2
            if feats_k is not None:
                g = torch.cat((ops.gather_patches(f, ids, C, per=B), ops.gather_patches(feats_k[li], ids, C, per=B)), dim=0)
            else:
                g = ops.gather_patches(f, ids, C, per=B)
            rows.append(netF.embed(g, li).split(2 * B * ids.shape[1]))     # (q rows, k rows): one cat in backward
            counts.append(ids.shape[1])
        T, monce = o.alg_cut_nce_T, o.alg_cut_nce_loss == "monce"
        tot = [0.0, 0.0]

        def one_set(Pl):
            ls = [i for i, c in enumerate(counts) if c == Pl]
            n = B * Pl
            q = torch.cat([rows[i][0] for i in ls], dim=0)                           # [layer][term][B * P_l] problems
            k = torch.cat([rows[i][1] for i in ls], dim=0)
            if self.hdce:      # problems [layer][term][B]: the NCE term (term 0) is weighted, the identity term only with alg_cut_MSE_idt (:734-766)
                wperiod, wcount = (1, 1) if self.hdce_idt_weighted else (2 * B, B)
                loss = ops.patch_hdce_loss(q, k, 2 * len(ls) * B, T, o.alg_cut_HDCE_gamma, wperiod, wcount).view(len(ls), 2, n)
            else:
                loss = ops.patch_nce_loss(q, k, 2 * len(ls) * B, T, P, monce).view(len(ls), 2, n)
            return loss.mean(dim=2).sum(dim=0) * o.alg_cut_lambda_NCE

        # (round 6, measured and removed: the smaller patch-count set on a forked third stream inside the graphs -- 20.0 -> 23.5 ms,
        #  profiles/r06_fork_nce_sets_ab.txt; like the third fork of the key-side encoder pass, a second fork costs the graph more than it hides)
        for Pl in sorted(set(counts)):
            m = one_set(Pl)
            tot = [tot[0] + m[0], tot[1] + m[1]]
        L = len(self.nce_layers)
        self.loss_G_NCE, self.loss_G_NCE_Y = tot[0] / L, tot[1] / L
        self.loss_G_tot = self.loss_G_tot + (self.loss_G_NCE + self.loss_G_NCE_Y) * 0.5 + self._pixel_losses()

    def _pixel_losses(self):
        """cut_model.py:771-786,823-833: the supervised term lambda_supervised * L1 | MSE(fake_B, real_B) (aligned data) and the identity term
        lambda_MSE_idt * L1(idt_B, real_B), both from ONE ops.pixel_loss call on `self.fake` = [fake_B | idt_B] (segment 0 / segment 1 against
        the same real_B: no slices, one autograd node, one backward launch).  Sets loss_G_supervised / loss_G_MSE_idt (device tensors) and
        returns their sum for loss_G_tot.  The reference adds the supervised term only if its value is > 0, a host read of a device scalar --
        a synchronisation, and illegal inside the captured generator graph; the sum is added unconditionally here: a term that is 0 has a zero
        gradient (sign(0) = 0, 2 * 0 = 0), so the update is the same.  With neither option set nothing is launched and 0 is returned."""
        o = self.opt
        mode_sup, mode_idt = self.pixel_modes
        if mode_sup == ops.PIXEL_OFF and mode_idt == ops.PIXEL_OFF:
            if o.alg_cut_MSE_idt:          # lambda_MSE_idt <= 0: the name is in loss_names, the value is 0
                self.loss_G_MSE_idt = torch.zeros((), device=self.device)
            return 0
        modes, lambdas = (mode_sup, mode_idt), (o.alg_cut_lambda_supervised, o.alg_cut_lambda_MSE_idt)
        S = 2 if o.alg_cut_nce_idt else 1
        losses = ops.pixel_loss(self.fake, self.real_B, o.model_output_nc, modes[:S], lambdas[:S])
        if mode_sup != ops.PIXEL_OFF:
            self.loss_G_supervised = losses[0]
        if o.alg_cut_MSE_idt:
            self.loss_G_MSE_idt = losses[1]
        return losses.sum()

    def compute_G_loss_cut(self):
        """cut_model.py:708-837 (NCE + identity NCE + the supervised / identity pixel terms)."""
        if self._batched_nce():
            return self.compute_G_loss_cut_batched()
        fq, fk = self.calculate_feats(self.real_A, self.fake_B)
        self.loss_G_NCE = self.calculate_NCE_loss(fq, fk, weighted=True) if self.opt.alg_cut_lambda_NCE > 0.0 else 0.0
        if self.opt.alg_cut_nce_idt and self.opt.alg_cut_lambda_NCE > 0.0:
            fq, fk = self.calculate_feats(self.real_B, self.idt_B)
            self.loss_G_NCE_Y = self.calculate_NCE_loss(fq, fk, weighted=self.hdce_idt_weighted)
            loss_NCE_both = (self.loss_G_NCE + self.loss_G_NCE_Y) * 0.5
        else:
            loss_NCE_both = self.loss_G_NCE
        self.loss_G_tot = self.loss_G_tot + loss_NCE_both + self._pixel_losses()

    def calculate_feats(self, src, tgt):
        """:848-887: q from the translated image, k from the source, SAME patch ids (drawn on the k pass)."""
        net = self._net("G_A")
        feat_q = net.get_feats(tgt, self.nce_layers)
        feat_k = net.get_feats(src, self.nce_layers)
        ids = None
        if self.patch_ids_injection is not None:
            ids = self.patch_ids_injection(self._feat_calls, [tuple(f.shape) for f in feat_k])
        self._feat_calls += 1
        netF = self._net("F")
        netF.arena.ensure_fresh()
        feat_k_pool, sample_ids = netF(feat_k, self.opt.alg_cut_num_patches, ids, self.feat_channels)
        feat_q_pool, _ = netF(feat_q, self.opt.alg_cut_num_patches, sample_ids, self.feat_channels)
        return feat_q_pool, feat_k_pool

    def calculate_NCE_loss(self, feat_q_pool, feat_k_pool, weighted=True):
        """:889-909.  `weighted` (SRC_hDCE only): the NCE(G(X), X) term runs with the hDCE weights, the identity term with weight=None unless
        alg_cut_MSE_idt is set (:734-766)."""
        total = 0.0
        for f_q, f_k, crit in zip(feat_q_pool, feat_k_pool, self.criterionNCE):
            loss = crit(feat_q=f_q, feat_k=f_k, current_batch=self.get_current_batch_size(), weighted=weighted) * self.opt.alg_cut_lambda_NCE
            total = total + loss.mean()
        return total / len(self.nce_layers)

    # ---- step driver (cut_step.py): which one ran the LAST optimize_parameters(): "sequential" (BaseModel's group loop), "early" (discriminator
    # half eager on a second stream) or "graph" (that half replayed from a hipGraph); `step_driver_note` holds the reason a faster driver was
    # not taken (bench.py and the driver-agreement tests report both)
    step_driver = "sequential"
    step_driver_note = ""

    def optimize_parameters(self):
        if not self.driver.early_D():
            self.step_driver = "sequential"
            if self.sem_cls != "off" and self.opt.isTrain:      # three groups: the early-D and captured drivers are built for [G, D]
                self.step_driver_note = "train_semantic_cls: the CLS group is a third network group; the step runs the groups in sequence"
            return super().optimize_parameters()
        self.driver.optimize_parameters()

    # ---- discriminator loss (base_gan_model.py:341-419) ------------------------------------------------------------------
    def get_current_APA_prob(self):
        """base_gan_model.py:329-339: APA_p / APA_adjust summed over the discriminators -- the one place that reads them on the host"""
        out = {"APA_p": 0.0, "APA_adjust": 0.0}
        for dn in self.discriminators_names:
            calc = getattr(self, dn + "_loss_calculator")
            out["APA_p"] += float(calc.adaptive_pseudo_augmentation_p)
            out["APA_adjust"] += float(calc.adjust)
        return out

    def _d_aug_draw(self, kind, index=0):
        return self.d_aug_injection(kind, index) if self.d_aug_injection is not None else None

    def draw_D_fakes(self, reader_stream=None):
        """The host-side half of compute_D_loss_generic (base_gan_model.py:341-365) for every discriminator, in the reference's draw order on
        the pool's RNG: `fake_B_pool.query` (of fake_B_noisy with dataaug_D_noise: cut_model.py:668-682, the pool stores noisy images), then with
        dataaug_APA `get_random` for the batch the flagged real samples come from.  Returns (fakes, alts or None), one entry per
        discriminator.  With both options off: the pool queries and nothing else."""
        src = self.fake_B
        if (self.d_noise > 0.0 or self.d_apa) and not (self.context and self.d_noise > 0.0):      # (framed + noisy: the forward drew the step's key)
            self._d_key = ops.d_aug_key(self.device) if self.d_aug_injection is None else None      # one Philox key per step
        if self.context:                # the forward's frame launch made the framed fake and its noisy copy: the pool stores framed images
            src = self.fake_B_with_context_noisy if self.d_noise > 0.0 else self.fake_B_with_context
        elif self.d_noise > 0.0:        # call index 0: the fake batch is drawn first, as in the reference
            (self.fake_B_noisy,), _ = ops.d_aug(self.fake_B, self.opt.model_output_nc, self.d_noise, z=self._d_aug_draw("z_fake"), key=self._d_key, call=0)
            src = self.fake_B_noisy
        fakes, alts = [], [] if self.d_apa else None
        for _ in self.discriminators_names:
            fakes.append(self.fake_B_pool.query(src, reader_stream=reader_stream).detach())
            if self.d_apa:
                alts.append(self.fake_B_pool.get_random(self.batch_size, reader_stream=reader_stream))
                self.APA_img = alts[-1]
        return fakes, alts

    def real_D_operands(self, alts, outs=None):
        """The real batch of every discriminator from ONE launch that reads real_B once: real_B + sigma z (call index 1, the same z for all of
        them) where unflagged, the discriminator's own `alts` entry where its flag is set (flag = u < its p, both on the device).  `outs`: the
        static operands of a captured graph, written in place.  Without APA all discriminators share one operand (`real_B_noisy`); with both
        options off this is real_B itself and nothing is launched."""
        n = len(self.discriminators_names)
        real = self.real_B_D            # with data_online_context_pixels: real_B_with_context, and every operand below has the framed shape
        if not (self.d_noise > 0.0 or self.d_apa):
            return [real] * n
        z = self._d_aug_draw("z_real") if self.d_noise > 0.0 else None
        if not self.d_apa:
            (noisy,), _ = ops.d_aug(real, self.opt.model_output_nc, self.d_noise, z=z, key=self._d_key, call=1, outs=outs)
            setattr(self, "real_B_with_context_noisy" if self.context else "real_B_noisy", noisy)
            return [noisy] * n
        calcs = [getattr(self, dn + "_loss_calculator") for dn in self.discriminators_names]
        us = [self._d_aug_draw("u", d) for d in range(n)]
        reals, flags = ops.d_aug(real, self.opt.model_output_nc, self.d_noise, z=z, key=self._d_key, call=1, alts=alts,
                                 ps=[c.apa_state[0:1] for c in calcs], us=None if us[0] is None else us, streams=[c.apa_stream for c in calcs], outs=outs)
        for d, c in enumerate(calcs):
            c.apa_flags = flags[d]
        return reals

    def compute_D_loss(self):
        """base_gan_model.py:341-419: every discriminator draws ITS OWN fake batch from the history pool (compute_D_loss_generic)."""
        tot = 0
        drawn = self.driver.drawn_fakes          # early-D driver: drawn before the fork (same draw order)
        fakes, alts = drawn if drawn is not None else self.draw_D_fakes()
        reals = self.real_D_operands(alts)
        self._dropout_seek(self.discriminators_names, 1)
        for i, dn in enumerate(self.discriminators_names):
            val = getattr(self, dn + "_loss_calculator").compute_loss_D(self._net(dn), reals[i], fakes[i], None)
            setattr(self, "loss_D_GAN_" + dn, val)
            tot = tot + val
        self.loss_D_tot = _ScaleGradFn.apply(tot, self.loss_scale)

    def _d_half_body(self, reals, fakes, its):
        """compute_D_loss + backward on given operands (the pool draws and the augmentations are the caller's)"""
        vals, tot = [], 0
        self._dropout_seek(self.discriminators_names, 1)
        for dn, real, fake in zip(self.discriminators_names, reals, fakes):
            val = getattr(self, dn + "_loss_calculator").compute_loss_D(self._net(dn), real, fake, None)
            vals.append(val)
            tot = tot + val
        tot = _ScaleGradFn.apply(tot, self.loss_scale)
        # round 6: the discriminators' weight gradients leave as grouped launches too (34 split-K launches of 37 - 69 us, each sized to fill
        # the chip by itself, next to the generator's backward); the spectral-norm fix of a discriminator flushes the ones it reads first
        with ops.deferred_wgrads():
            (tot / its).backward()
        return vals, tot
