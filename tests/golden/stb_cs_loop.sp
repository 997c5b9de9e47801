* self-biased common-source stage: the drain feeds the gate through the 0 V probe and an R-C-R-C network, NMOS
VDD vdd 0 DC 3
Vprobe d fb DC 0
RD vdd d 2k
R1 fb n1 10k
C1 n1 0 1p
R2 n1 g 10k
C2 g 0 1p
CL d 0 10p
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.stb Vprobe dec 10 1k 10g
